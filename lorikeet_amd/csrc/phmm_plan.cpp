// Launch planner of the MI355X PairHMM engine (phmm_plan.hpp): bins the regions of a batch into kernel shape classes <L lanes
// per pair, K haplotype columns per lane>, cuts the chained classes into work items and orders them for the launch.  Host
// arithmetic on the offset arrays only: no device is touched here.
#include "phmm_plan.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <map>
#include <tuple>

#include "phmm_host.hpp"

using namespace phmm;

namespace phmm_plan {
namespace {

#ifndef PHMM_MIXED_RUNS
#define PHMM_MIXED_RUNS 32
#endif
constexpr unsigned kMixedRunsPerSlot = PHMM_MIXED_RUNS;  // runs per wave slot of a mixed batch (see run_lengths)

constexpr uint64_t kGenericScratchBytes = 1ull << 30;

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int round_up_k(int k) {
    for (int i = 0; i < kNumInstantiatedK; ++i)
        if (kInstantiatedK[i] >= k) return kInstantiatedK[i];
    return 0;
}

// Registers cap the resident waves per SIMD (3*K f64 of DP state per lane dominates; K <= 25 is
// compiled for 2 waves, PHMM_TWO_WAVE_MAX_K).
int waves_per_simd(int K) { return K <= 25 ? 2 : 1; }

// Throughput model of a region under <L,K>, calibrated on MI355X (tools/shapes.py): useful fraction of
// issued lane-steps x the per-step overhead (DPP shifts, LDS fetch, loop: ~11 of 7*K+11 VALU ops per
// step) x the issue rate one resident wave reaches alone (a wave issues a VALU op every ~6 clk, two waves
// together one every ~4.7: tools/ubench/issue.hip; measured 0.81 on <16,25>).
// Chained kernel at 16 lanes per pair: the four haplotype slots of a wave can be shared by S = 1, 2 or 4 streams of
// reads (phmm_chain_kernels.hip), so any haplotype count fills them.  Every extra stream costs row-producer work
// (rows are built per stream, in shorter ticks): measured 3990 / 3700 / 3300 GCUPS at 1 / 2 / 4 streams with all
// slots busy, i.e. ~6 % per extra stream.  Returns S, and the slot fill (times that factor) it achieves.
int chain_streams(uint32_t nh, double *fill_out) {
    int best_s = 1;
    double best = 0.0;
    for (int S : {1, 2, 4}) {
        const uint32_t gs = 4 / S;
        const double fill = (double)nh / (double)(((nh + gs - 1) / gs) * gs) * (1.0 - 0.06 * (S - 1));
        if (fill > best + 1e-9) {
            best = fill;
            best_s = S;
        }
    }
    if (fill_out) *fill_out = best;
    return best_s;
}

double shape_efficiency(int L, int K, uint32_t nh, uint32_t mean_r, uint32_t max_h, bool chained) {
    const int G = WAVE / L;
    double hap_fill = (double)nh / (double)(((nh + G - 1) / G) * G);
    if (chained && L == 16) (void)chain_streams(nh, &hap_fill);
    // fill / drain steps of the lane pipeline: per read, or (chained kernel) amortised over a run of reads
    const double ramp = chained ? 1.0 : (double)std::max<uint32_t>(mean_r, 1) / (double)(std::max<uint32_t>(mean_r, 1) + L - 1);
    const double col_fill = (double)max_h / (double)(L * K);
    const double step = 7.0 * K / (7.0 * K + 11.0);
    const double occ = waves_per_simd(K) >= 2 ? 1.0 : 0.84;
    return hap_fill * ramp * col_fill * step * occ;
}

double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- 1: per-region shape, totals ----------------------------------------------------------------
struct RegionShape {
    uint32_t nr, nh, max_r, max_h, mean_r, min_r = 0xffffffffu, min_h = 0xffffffffu;
    uint64_t cells;
};

std::vector<RegionShape> region_shapes(const BatchOffsets &o, BatchPlan &plan) {
    std::vector<RegionShape> shape(o.n_regions);
    plan.read_region.resize(plan.n_reads);
    for (uint32_t g = 0; g < o.n_regions; ++g) {
        RegionShape s{};
        s.nr = o.region_read_off[g + 1] - o.region_read_off[g];
        s.nh = o.region_hap_off[g + 1] - o.region_hap_off[g];
        uint64_t sum_r = 0, sum_h = 0;
        for (uint32_t r = o.region_read_off[g]; r < o.region_read_off[g + 1]; ++r) {
            const uint32_t len = o.read_off[r + 1] - o.read_off[r];
            s.max_r = std::max(s.max_r, len);
            s.min_r = std::min(s.min_r, len);
            sum_r += len;
            plan.read_region[r] = g;
        }
        for (uint32_t a = o.region_hap_off[g]; a < o.region_hap_off[g + 1]; ++a) {
            const uint32_t len = o.hap_off[a + 1] - o.hap_off[a];
            s.max_h = std::max(s.max_h, len);
            s.min_h = std::min(s.min_h, len);
            sum_h += len;
        }
        s.mean_r = s.nr ? (uint32_t)(sum_r / s.nr) : 0;
        s.cells = sum_r * sum_h;
        plan.cells += s.cells;
        plan.alg_bytes += 5 * sum_r + sum_h + 8ull * s.nr * s.nh;
        shape[g] = s;
    }
    return shape;
}

// ---- 2: choose <L,K> per region -----------------------------------------------------------------
// Candidates L in {16,32,64}; K = ceil(max_h / L) rounded up to an instantiated value.
// Pick the most efficient one, then trade lanes-per-pair for more waves while the batch is
// too small to fill the chip.
// The chained kernel holds a 19 KB LDS ring per wave (two waves per SIMD): a win wherever the per-read kernel
// runs two waves per SIMD anyway, a loss against the three or four waves small K gets at 32 / 64 lanes per
// pair (measured: <32,10> 3150 per-read vs 2860 chained; <32,13> 3030 vs 3450; <32,19> 3220 vs 3470).
bool chain_forced(const Switches &sw) { return sw.force_chain >= 0; }  // tests: every chainable shape chains
bool chain_shape_ok(int L, int k, const RegionShape &s, const Switches &sw) {
    return k > 0 && k <= chain_max_k() && (L == 16 || k >= 13 || chain_forced(sw)) && s.min_r >= 1 && s.min_h >= 1 &&
           s.nh <= 0xffffu /* ChainItem::quad */;
}

// (`assume_chain`: second planning pass -- the batch is large enough for the chained kernel)
void pick(const RegionShape &s, int min_L, const Switches &sw, bool assume_chain, int &L_out, int &K_out) {
    double best = -1.0;
    L_out = 0;
    K_out = 0;
    for (int L : {16, 32, 64}) {
        if (L < min_L) continue;
        if (sw.force_L && L != sw.force_L) continue;
        const int k = round_up_k((int)((std::max<uint32_t>(s.max_h, 1) + L - 1) / L));
        if (!k) continue;
        const double e = shape_efficiency(L, k, s.nh, s.mean_r, s.max_h, assume_chain && chain_shape_ok(L, k, s, sw));
        if (e > best) {
            best = e;
            L_out = L;
            K_out = k;
        }
    }
}

struct ShapeChoice {
    std::vector<int> L, K;  // per region: lanes per pair and columns per lane; -1 = nothing to do, 0 = generic kernel
    int min_L = 16;
};

ShapeChoice plan_shapes(const std::vector<RegionShape> &shape, const Switches &sw, uint32_t gpu_sharers, bool assume_chain) {
    const uint32_t n_regions = (uint32_t)shape.size();
    ShapeChoice c;
    c.L.resize(n_regions);
    c.K.resize(n_regions);
    for (;;) {
        uint64_t waves = 0;
        for (uint32_t g = 0; g < n_regions; ++g) {
            const RegionShape &s = shape[g];
            if (!s.nr || !s.nh) {
                c.L[g] = c.K[g] = -1;  // nothing to do
                continue;
            }
            pick(s, c.min_L, sw, assume_chain, c.L[g], c.K[g]);
            if (c.L[g]) waves += (uint64_t)s.nr * ((s.nh + WAVE / c.L[g] - 1) / (WAVE / c.L[g]));
        }
        // one wave per SIMD is enough to stop trading lanes for waves (measured on 1, 2, 4 regions of config 2:
        // <64,5> 41 us, <32,10> 54 us vs <64,5> 60 us, <16,19> 87 us vs <32,10> 88 us)
        if (waves * gpu_sharers >= 1ull * kNumSimd || c.min_L == 64 || sw.force_L) break;
        c.min_L *= 2;
    }
    return c;
}

// ---- 3: chained or per read ---------------------------------------------------------------------
// Chained kernel (phmm_chain_kernels.hip): reads of a region stream back to back through the lane
// pipeline, which removes the per-read fill/drain steps.  Worth it (and balanced) only when there is
// enough work to give every wave a run of reads: decide per batch, qualify per region.
int streams_of(int L, uint32_t nh, int force_streams /* tests: 1 | 2 | 4 */) {
    if (L != 16) return 1;
    if (force_streams == 1 || force_streams == 2 || force_streams == 4) return force_streams;
    return chain_streams(nh, nullptr);
}

// wave-sweeps (one read against one wave-load of haplotypes) under the chosen shapes
uint64_t count_units(const std::vector<RegionShape> &shape, const ShapeChoice &c, int force_streams) {
    uint64_t u = 0;
    for (uint32_t g = 0; g < (uint32_t)shape.size(); ++g)
        if (c.L[g] > 0) {
            const uint32_t S = (uint32_t)streams_of(c.L[g], shape[g].nh, force_streams), gs = (uint32_t)(WAVE / c.L[g]) / S;
            u += (uint64_t)shape[g].nr * ((shape[g].nh + gs - 1) / gs) / S;
        }
    return u;
}

// run length: about eight runs per wave slot (balance), but never runs shorter than four reads (measured on 128
// regions of config 2: runs of 2 reads 3380, of 4 reads 3530, per-read kernel 3450 GCUPS); below two runs of two
// per slot the batch stays with the per-read kernel
uint32_t runs_for(uint64_t u) {
    const uint32_t r = (uint32_t)std::min<uint64_t>(CHAIN_MAX_READS, u / (8ull * 2 * kNumSimd));
    return r >= 2 && r < 4 ? 4u : r;
}

struct ChainDecision {
    ShapeChoice shapes;
    uint64_t units = 0;
    uint32_t chain_reads = 0;  // reads per run of a uniform batch; below 2: the batch stays with the per-read kernel
    bool chainable(uint32_t g, const RegionShape &s, const Switches &sw) const {
        return chain_reads >= 2 && shapes.L[g] > 0 && chain_shape_ok(shapes.L[g], shapes.K[g], s, sw);
    }
};

ChainDecision decide_chain(const std::vector<RegionShape> &shape, const Switches &sw, uint32_t gpu_sharers) {
    ChainDecision d;
    d.shapes = plan_shapes(shape, sw, gpu_sharers, false);
    d.units = count_units(shape, d.shapes, sw.force_streams);
    d.chain_reads = runs_for(d.units);
    if (chain_forced(sw)) d.chain_reads = (uint32_t)std::min(CHAIN_MAX_READS, sw.force_chain);
    if (d.chain_reads >= 2 && !sw.force_L) {
        // chained sweeps pay no per-read fill/drain: choose the shapes again without that term (more lanes per pair
        // become attractive for regions with few haplotypes), and keep the result if the batch still chains
        ShapeChoice again = plan_shapes(shape, sw, gpu_sharers, true);
        const uint64_t units = count_units(shape, again, sw.force_streams);
        const uint32_t cr = chain_forced(sw) ? d.chain_reads : runs_for(units);
        if (cr >= 2 && again.min_L == 16) {
            d.chain_reads = cr;
            d.units = units;
            d.shapes = std::move(again);
        } else {
            d.shapes.min_L = again.min_L;  // (PHMM_TRACE prints the last pass's)
        }
    }
    return d;
}

// ---- 4: regions of one <L, K, kernel> form a class ------------------------------------------------
using ClassMap = std::map<std::tuple<int, int, int>, ShapeClass>;  // (L, K, 0 = per-read kernel | streams of the chained kernel)

ClassMap group_classes(const BatchOffsets &o, const std::vector<RegionShape> &shape, const ChainDecision &d, const Switches &sw) {
    ClassMap by_shape;
    for (uint32_t g = 0; g < o.n_regions; ++g) {
        if (d.shapes.L[g] < 0) continue;
        const RegionShape &s = shape[g];
        int L = d.shapes.L[g], K = d.shapes.K[g];
        // LDS staging must hold the longest read of the region, one wave per block at least
        const size_t rows = align_up((size_t)s.max_r + 1, 8);
        if (L && rows * LDS_ROW_BYTES > kLdsBytesPerCU) L = K = 0;
        const bool chain = L && d.chainable(g, s, sw);
        const int streams = chain ? streams_of(d.shapes.L[g], s.nh, sw.force_streams) : 1;
        ShapeClass &c = by_shape[std::make_tuple(L, K, chain ? streams : 0)];
        c.L = L;
        c.K = K;
        c.chain = chain;
        c.streams = streams;
        if (chain) c.regions.push_back(g);
        for (uint32_t r = o.region_read_off[g]; r < o.region_read_off[g + 1]; ++r) c.reads.push_back(r);
        c.max_r = std::max(c.max_r, s.max_r);
        c.max_h = std::max(c.max_h, s.max_h);
        if (L) c.max_quads = std::max(c.max_quads, (s.nh + WAVE / L - 1) / (WAVE / L));
        c.cells += s.cells;
        if (!L)
            for (uint32_t r = o.region_read_off[g]; r < o.region_read_off[g + 1]; ++r) c.pair_first.push_back(s.nh);
    }
    return by_shape;
}

// ---- 5: reads per run, per region of a chained class ----------------------------------------------
// Reads per run.  Uniform batches get `chain_reads` (about eight runs per wave slot), mixed ones a quarter of that (below).
// Scaling a region's count by its cost per read -- (rows + SUM + RESET) x (7 VALU per column + ~11 per step) relative to
// the batch's mean, so that every work item costs about the same -- looked right and measured wrong once the items were
// sorted by cost and spread over the XCDs (1 536 mixed regions: 17.4 ms with it, 16.8 without): short runs of expensive
// reads pay the pipeline's fill more often than they save at the tail.
std::vector<uint32_t> run_lengths(const ClassMap &by_shape, uint32_t n_regions, const ChainDecision &d, const Switches &sw) {
    std::vector<uint32_t> reg_run(n_regions, 0);
    // A uniform batch balances with eight equal runs per wave slot; a mix of classes does not -- its items differ in
    // cost whatever the estimate, and the launch ends when the last long item does.  Mixed batches therefore get runs
    // a quarter as long (32 per slot, never below 4 reads): 1 536 mixed regions 20.4 -> 16.9 ms.
    size_t n_chain_classes = 0;
    for (const auto &kv : by_shape) n_chain_classes += kv.second.chain ? 1 : 0;
    uint32_t base_reads = d.chain_reads;
    if (n_chain_classes > 1 && !chain_forced(sw))
        base_reads = std::max<uint32_t>(4, std::min<uint32_t>(d.chain_reads, (uint32_t)(d.units / ((uint64_t)kMixedRunsPerSlot * 2 * kNumSimd))));
    for (const auto &kv : by_shape)
        if (kv.second.chain)
            for (uint32_t g : kv.second.regions)
                reg_run[g] = std::min<uint32_t>(CHAIN_MAX_READS, base_reads * (uint32_t)kv.second.streams);
    return reg_run;
}

// ---- 6: work items and launch geometry of one class -----------------------------------------------
void make_chain_items(ShapeClass &c, const BatchOffsets &o, const std::vector<RegionShape> &shape, const std::vector<uint32_t> &reg_run,
                      const Switches &sw, unsigned flags) {
    for (uint32_t g : c.regions) {
        const uint32_t r0 = o.region_read_off[g], r1 = o.region_read_off[g + 1];
        const uint32_t gs = (uint32_t)(WAVE / c.L) / (uint32_t)c.streams;  // haplotypes per work item
        const uint32_t nq = (shape[g].nh + gs - 1) / gs;
        const uint32_t run = reg_run[g];
        // the haplotype groups of one run next to each other: they sweep the same read bytes, and items that are
        // launched together find them in L2 (config 3, 10 000 regions: HBM traffic 2.7 x the algorithmic bytes
        // with the groups a whole pass apart)
        // A haplotype count that leaves the last wave of a one-stream class partly empty (5 haplotypes: 4 + 1) gives
        // the remainder to items of its own with 2 or 4 streams of reads, which fill the wave's slots with the same
        // haplotypes again (chain_streams): 5 haplotypes 0.63 -> 0.96 of the slots busy, 9: 0.75 -> 0.98.
        uint32_t nq_main = nq, rest = 0, rest_streams = 1;
        if (c.streams == 1 && c.L == 16 && !(flags & PHMM_FLAG_F32_FIRST) && sw.force_streams == 0 && shape[g].nh > 4 && shape[g].nh % 4 != 0) {
            rest = shape[g].nh % 4;
            rest_streams = (uint32_t)chain_streams(rest, nullptr);
            if (rest_streams > 1) nq_main = shape[g].nh / 4;
            else rest = 0;
        }
        for (uint32_t r = r0; r < r1; r += run)
            for (uint32_t q = 0; q < nq_main; ++q)
                c.chain_items.push_back(ChainItem{g, (uint16_t)q, (uint8_t)c.K, (uint8_t)c.streams, r, std::min(r1, r + run)});
        if (rest) {
            const uint32_t gs2 = 4 / rest_streams, q0 = nq_main * 4 / gs2, nq2 = (rest + gs2 - 1) / gs2;
            const uint32_t run2 = std::min<uint32_t>(CHAIN_MAX_READS, run * rest_streams);
            for (uint32_t r = r0; r < r1; r += run2)
                for (uint32_t q = 0; q < nq2; ++q)
                    c.chain_items.push_back(ChainItem{g, (uint16_t)(q0 + q), (uint8_t)c.K, (uint8_t)rest_streams, r, std::min(r1, r + run2)});
        }
    }
    // (the launch is ordered longest item first below, across all classes: one sort there instead of one per class and
    // another over the whole -- the planner of a 186-region chunk of the ragged mix spent 1.3 of its 2.6 ms here)
}

void finish_class(ShapeClass &c, const BatchOffsets &o, const std::vector<RegionShape> &shape, const std::vector<uint32_t> &reg_run,
                  const Switches &sw, unsigned flags, uint32_t n_reads) {
    const uint32_t n_items = (uint32_t)c.reads.size();
    c.identity = (n_items == n_reads);
    for (uint32_t i = 0; c.identity && i < n_items; ++i) c.identity = (c.reads[i] == i);
    if (c.chain) {
        make_chain_items(c, o, shape, reg_run, sw, flags);
        c.f32_first = (flags & PHMM_FLAG_F32_FIRST) && (c.L == 16 || c.L == 32);
        if (c.f32_first) {  // the f64 per-read kernel runs behind the f32 sweep over the reads it flags
            c.lds_rows = (uint32_t)align_up((size_t)c.max_r + 1, 8);
            c.waves_per_block = 1;
            c.lds_bytes = (size_t)c.lds_rows * LDS_ROW_BYTES;
            c.grid = dim3(n_items, 1, 1);  // one wave per read, it walks all haplotype groups
            c.cnd_select = 0;
        }
        const char *f32 = c.f32_first ? "_f32" : "";
        if (c.streams > 1)
            snprintf(c.name, sizeof c.name, "phmm_forward_chain%s<%d,%d> x%d streams", f32, c.L, c.K, c.streams);
        else
            snprintf(c.name, sizeof c.name, "phmm_forward_chain%s<%d,%d>", f32, c.L, c.K);
    } else if (c.L) {
        c.lds_rows = (uint32_t)align_up((size_t)c.max_r + 1, 8);
        const size_t per_wave = (size_t)c.lds_rows * LDS_ROW_BYTES;
        // One wave per workgroup: waves are independent (no barrier, private LDS), and a multi-wave block
        // would hold its LDS until its longest read finishes -- with mixed read lengths that idles SIMDs.
        c.waves_per_block = 1;
        c.lds_bytes = per_wave * c.waves_per_block;
        // Enough reads to fill the chip -> one wave walks all haplotype groups of its read (row
        // constants staged once); otherwise spread the groups over gridDim.y.
        bool split = (uint64_t)n_items < 4ull * kNumSimd;
        c.grid = dim3((n_items + c.waves_per_block - 1) / c.waves_per_block, split ? c.max_quads : 1, 1);
        // a wave alone on its SIMD is latency-bound: the v_cndmask select (one more VALU op, no EXEC round
        // trip) is ~8 % faster there; with two resident waves the EXEC-masked select wins
        const uint64_t waves = (uint64_t)n_items * (split ? c.max_quads : 1);
        c.cnd_select = waves < 2ull * kNumSimd ? 1u : 0u;
        snprintf(c.name, sizeof c.name, "phmm_forward<%d,%d>", c.L, c.K);
    } else {
        // generic: exclusive prefix of pairs per read, scratch for a bounded grid
        uint64_t acc = 0;
        for (auto &v : c.pair_first) {
            const uint64_t nh = v;
            v = acc;
            acc += nh;
        }
        c.pair_first.push_back(acc);
        const uint64_t per_thread = 6ull * (c.max_h + 1) * sizeof(double);
        uint64_t threads = std::min<uint64_t>(align_up(acc, 256), 1024ull * 256);
        threads = std::min<uint64_t>(threads, std::max<uint64_t>(256, kGenericScratchBytes / per_thread / 256 * 256));
        c.generic_blocks = (uint32_t)(threads / 256);
        c.generic_scratch_bytes = threads * per_thread;
        snprintf(c.name, sizeof c.name, "phmm_forward_generic");
    }
}

// the chained classes of one lanes-per-pair value (and one precision) share a launch
void join_chain_group(std::vector<ChainGroup> &groups, const ShapeClass &c) {
    ChainGroup *grp = nullptr;
    for (auto &gq : groups)
        if (gq.L == c.L && gq.f32 == c.f32_first) grp = &gq;
    if (!grp) {
        groups.emplace_back();
        grp = &groups.back();
        grp->L = c.L;
        grp->f32 = c.f32_first;
    }
    grp->items.insert(grp->items.end(), c.chain_items.begin(), c.chain_items.end());
}

// ---- 7: what the launches sweep -------------------------------------------------------------------
// What these launches sweep, padding and all (phmm_batch_executed_cells), in lane-cells = steps x 64 lanes x K columns per
// wave, and where the padding comes from: columns beyond a haplotype's end (16 K - H), haplotype slots a wave leaves
// empty, and steps that carry no read row (the SUM / RESET rows between the reads of a run, the L - 1 steps a run needs to
// reach its last lane, the rows the longest of a wave's streams has more than the others).
void account_swept(BatchPlan &plan, const BatchOffsets &o, const std::vector<RegionShape> &shape, bool trace) {
    const uint32_t *read_off = o.read_off;
    uint64_t swept = 0, pad_cols = 0, pad_slots = 0, t_marks = 0, t_fill = 0, t_uneven = 0, t_uneven_best = 0;  // (t_*: PHMM_TRACE only)
    auto haps_of = [&o](uint32_t g, uint32_t first, uint32_t slots, uint32_t lanes_cols, uint64_t &sum_h, uint32_t &valid) {
        const uint32_t h0 = o.region_hap_off[g], nh = o.region_hap_off[g + 1] - h0;
        sum_h = 0;
        valid = 0;
        for (uint32_t a = first; a < first + slots && a < nh; ++a) {
            sum_h += std::min<uint32_t>(o.hap_off[h0 + a + 1] - o.hap_off[h0 + a], lanes_cols);
            ++valid;
        }
    };
    for (const auto &grp : plan.chain_groups)
        for (const ChainItem &x : grp.items) {
            const uint32_t S = std::max<uint32_t>(1, x.streams), L = (uint32_t)grp.L, GS = (64u / L) / S, LK = L * x.k;
            const uint32_t n = x.read_end - x.read_begin, n_sub = (n + S - 1) / S;
            uint64_t longest = 0, read_rows = 0;
            for (uint32_t st = 0; st < S; ++st) {  // (stream st sweeps reads [st n_sub, (st + 1) n_sub) of the run)
                const uint32_t lo = std::min(n, st * n_sub), hi = std::min(n, lo + n_sub);
                const uint64_t rows = read_off[x.read_begin + hi] - read_off[x.read_begin + lo];
                read_rows += rows;
                longest = std::max<uint64_t>(longest, rows + 2ull * (hi - lo));
            }
            const uint64_t steps = (longest + L) & ~1ull;
            swept += steps * 64ull * x.k;
            t_marks += 2ull * n * GS * LK;                                          // the SUM / RESET rows of its reads
            t_fill += (steps - longest) * 64ull * x.k;                              // reaching the last lane
            t_uneven += (longest * S - read_rows - 2ull * n) * (uint64_t)GS * LK;   // streams shorter than the longest
            if (trace && S > 1) {  // ... and what the best cut of the run into S contiguous parts would leave of that
                uint64_t lo_b = 0, hi_b = read_rows + 2ull * n;
                for (uint32_t i = 0; i < n; ++i) lo_b = std::max<uint64_t>(lo_b, read_off[x.read_begin + i + 1] - read_off[x.read_begin + i] + 2);
                while (lo_b < hi_b) {
                    const uint64_t mid = (lo_b + hi_b) / 2;
                    uint32_t parts = 1;
                    uint64_t acc = 0;
                    for (uint32_t i = 0; i < n; ++i) {
                        const uint64_t len = read_off[x.read_begin + i + 1] - read_off[x.read_begin + i] + 2;
                        if (acc + len > mid) {
                            ++parts;
                            acc = 0;
                        }
                        acc += len;
                    }
                    if (parts <= S) hi_b = mid; else lo_b = mid + 1;
                }
                t_uneven_best += (lo_b * S - read_rows - 2ull * n) * (uint64_t)GS * LK;
            }
            uint64_t sum_h;
            uint32_t valid;
            haps_of(x.region, (uint32_t)x.quad * GS, GS, LK, sum_h, valid);
            pad_cols += read_rows * ((uint64_t)valid * LK - sum_h);
            pad_slots += read_rows * (uint64_t)(GS - valid) * LK;
        }
    for (const auto &c : plan.classes) {
        if (c.chain) continue;  // (counted above; the f64 redo behind an f32 sweep touches the reads it flags only)
        if (!c.L) {
            swept += c.cells;
            continue;
        }
        const size_t n = c.identity ? plan.n_reads : c.reads.size();
        const uint32_t per_wave = 64u / (uint32_t)c.L, LK = (uint32_t)(c.L * c.K);
        for (size_t i = 0; i < n; ++i) {
            const uint32_t r = c.identity ? (uint32_t)i : c.reads[i], g = plan.read_region[r];
            const uint32_t quads = (shape[g].nh + per_wave - 1) / per_wave;
            const uint64_t rows = read_off[r + 1] - read_off[r];
            swept += (rows + (uint64_t)c.L - 1) * quads * 64ull * (uint64_t)c.K;
            for (uint32_t qd = 0; qd < quads; ++qd) {
                uint64_t sum_h;
                uint32_t valid;
                haps_of(g, qd * per_wave, per_wave, LK, sum_h, valid);
                pad_cols += rows * ((uint64_t)valid * LK - sum_h);
                pad_slots += rows * (uint64_t)(per_wave - valid) * LK;
            }
        }
    }
    if (trace)
        fprintf(stderr, "phmm plan: swept %.4e lane-cells for %.4e cells: columns %.4e, slots %.4e; chained items' SUM / RESET rows %.4e, fill %.4e, uneven streams %.4e (cut by rows: %.4e)\n",
                (double)swept, (double)plan.cells, (double)pad_cols, (double)pad_slots, (double)t_marks, (double)t_fill, (double)t_uneven, (double)t_uneven_best);
    plan.swept_cells = swept;
    plan.pad_column_cells = pad_cols;
    plan.pad_slot_cells = pad_slots;
}

// ---- 8: the order of a launch's items ---------------------------------------------------------------
void order_group(ChainGroup &grp, const uint32_t *read_off) {
    // longest item first across all classes of the launch: (rows of the run + its SUM / RESET rows) x the cost of a
    // step at the item's K (7 VALU per column + ~11 per step)
    const int L = grp.L;
    auto cost = [read_off, L](const ChainItem &x) {
        return (uint64_t)(read_off[x.read_end] - read_off[x.read_begin] + 2 * (x.read_end - x.read_begin) + L) *
               (uint64_t)(7 * x.k + 11);
    };
    {   // (keys made once -- the comparator used to fetch four offsets per comparison -- and unique, so a plain sort keeps
        // items of equal cost in the order they were made: the groups of a run stay next to each other)
        const size_t n = grp.items.size();
        std::vector<uint64_t> cst(n);
        uint64_t top = 0;
        for (size_t i = 0; i < n; ++i) top = std::max(top, cst[i] = cost(grp.items[i]));
        std::vector<uint32_t> idx(n), tmp(n);
        for (size_t i = 0; i < n; ++i) idx[i] = (uint32_t)i;
        if (top < (1ull << 33)) {  // LSD radix sort, descending, 11 bits a pass (stable): tens of microseconds for 10^4 items
            for (int shift = 0; (top >> shift) != 0; shift += 11) {
                uint32_t count[2049] = {0};
                for (size_t i = 0; i < n; ++i) count[2047 - ((cst[idx[i]] >> shift) & 2047) + 1] += 1;
                for (int d = 0; d < 2048; ++d) count[d + 1] += count[d];
                for (size_t i = 0; i < n; ++i) tmp[count[2047 - ((cst[idx[i]] >> shift) & 2047)]++] = idx[i];
                idx.swap(tmp);
            }
        } else {
            std::stable_sort(idx.begin(), idx.end(), [&cst](uint32_t x, uint32_t y) { return cst[x] > cst[y]; });
        }
        std::vector<ChainItem> sorted(n);
        for (size_t i = 0; i < n; ++i) sorted[i] = grp.items[idx[i]];
        grp.items.swap(sorted);
    }
    // XCD-aware placement.  The haplotype groups of one run (same region, same reads: equal cost, so the stable sort
    // left them next to each other) sweep the same read bytes.  Workgroups are dealt to the eight XCDs round robin,
    // each XCD with an L2 of its own, so neighbours in the launch never share one: take eight runs at a time and
    // emit their first groups, then their second groups, ... -- the groups of a run are then 8 blocks apart, on
    // the same XCD, started together.
    {
        std::vector<ChainItem> out;
        out.reserve(grp.items.size());
        auto same_run = [](const ChainItem &x, const ChainItem &y) {
            return x.region == y.region && x.read_begin == y.read_begin && x.read_end == y.read_end;
        };
        size_t i = 0;
        const size_t n = grp.items.size();
        while (i < n) {
            size_t start[9], len[8];  // up to eight consecutive runs
            int nr = 0;
            size_t j = i;
            while (nr < 8 && j < n) {
                size_t e = j + 1;
                while (e < n && same_run(grp.items[j], grp.items[e])) ++e;
                start[nr] = j;
                len[nr] = e - j;
                ++nr;
                j = e;
            }
            size_t longest = 0;
            for (int r = 0; r < nr; ++r) longest = std::max(longest, len[r]);
            for (size_t q = 0; q < longest; ++q)
                for (int r = 0; r < nr; ++r)
                    if (q < len[r]) out.push_back(grp.items[start[r] + q]);
            i = j;
        }
        grp.items.swap(out);
    }
    grp.single_k = grp.items.empty() ? 0 : grp.items[0].k;
    for (const ChainItem &it : grp.items)
        if (it.k != grp.single_k) {
            grp.single_k = 0;
            break;
        }
}

// ---- 9: one launch per range of K -------------------------------------------------------------------
// A mixed f64 group goes out as one launch per RANGE of K (the kernel of a range holds only its bodies: no spilled
// scalar registers, no scratch); the launches of a batch run side by side on parallel streams (phmm_batch_launch).
std::vector<ChainGroup> split_by_k_range(std::vector<ChainGroup> &&groups, const uint32_t *read_off) {
    std::vector<ChainGroup> split;
    for (auto &grp : groups) {
        if (grp.f32 || grp.single_k != 0 || grp.items.empty()) {
            split.push_back(std::move(grp));
            continue;
        }
        ChainGroup part[kChainRanges];
        for (const ChainItem &it : grp.items) part[chain_range_of(it.k)].items.push_back(it);  // (order kept: longest first)
        for (int r = 0; r < kChainRanges; ++r) {
            if (part[r].items.empty()) continue;
            part[r].L = grp.L;
            part[r].f32 = false;
            part[r].single_k = part[r].items[0].k;
            for (const ChainItem &it : part[r].items)
                if (it.k != part[r].single_k) {
                    part[r].single_k = -(r + 1);
                    break;
                }
            split.push_back(std::move(part[r]));
        }
    }
    // the heaviest launch first (it starts on the caller's stream, the others join it from the side streams)
    auto weight = [read_off](const ChainGroup &g) {
        uint64_t w = 0;
        for (const ChainItem &x : g.items) w += (uint64_t)(read_off[x.read_end] - read_off[x.read_begin]) * (uint64_t)(7 * x.k + 11);
        return w;
    };
    std::stable_sort(split.begin(), split.end(), [&weight](const ChainGroup &x, const ChainGroup &y) { return weight(x) > weight(y); });
    return split;
}

// ---- 10: the dominant class under its kernel's name -------------------------------------------------
// the dominant class under the name of the kernel that runs it (what rocprofv3 reports): the body alone for a launch
// whose items share one K, the kernel of its range of K otherwise
std::string dominant_kernel(const BatchPlan &plan, std::string dominant /* the heaviest class by its own name */) {
    for (const auto &c : plan.classes) {
        if (!c.chain || dominant != c.name) continue;
        for (const auto &grp : plan.chain_groups) {
            if (grp.L != c.L || grp.f32 != c.f32_first) continue;
            char nm[64] = {0};
            if (grp.f32) {
                if (grp.single_k == c.K) snprintf(nm, sizeof nm, "phmm_forward_chain_f32<%d,%d>", c.L, c.K);
                else if (grp.single_k == 0) snprintf(nm, sizeof nm, "phmm_forward_chain_f32_any<%d> (K = %d)", c.L, c.K);
            } else if (grp.single_k == c.K) {
                snprintf(nm, sizeof nm, "phmm_forward_chain_k<%d,%d>", c.L, c.K);
            } else if (grp.single_k < 0 && chain_range_of(c.K) == -grp.single_k - 1) {
#define PHMM_RANGE(R, LO, HI) \
    if (R == -grp.single_k - 1) snprintf(nm, sizeof nm, "phmm_forward_chain<%d,%d,%d> (K = %d)", c.L, LO, HI, c.K);
                PHMM_CHAIN_RANGES(PHMM_RANGE)
#undef PHMM_RANGE
            }
            if (nm[0]) {
                dominant = nm;
                if (c.streams > 1) dominant += " x" + std::to_string(c.streams) + " streams";
                break;
            }
        }
        break;
    }
    return dominant;
}

}  // namespace

BatchPlan plan_batch(const BatchOffsets &o, const Switches &sw, unsigned flags, uint32_t gpu_sharers) {
    BatchPlan plan;
    plan.n_regions = o.n_regions;
    plan.n_reads = o.region_read_off[o.n_regions];
    plan.n_haps = o.region_hap_off[o.n_regions];
    double marks[6] = {now_us()};
    int n_marks = 1;
    auto mark = [&marks, &n_marks] { marks[n_marks++] = now_us(); };

    const std::vector<RegionShape> shape = region_shapes(o, plan);
    mark();  // 1: shapes
    const ChainDecision d = decide_chain(shape, sw, gpu_sharers);
    if (sw.trace)
        fprintf(stderr, "phmm plan: %u regions, min_L %d, units %llu, chain_reads %u, region0 <%d,%d> chainable %d\n", o.n_regions,
                d.shapes.min_L, (unsigned long long)d.units, d.chain_reads, o.n_regions ? d.shapes.L[0] : 0, o.n_regions ? d.shapes.K[0] : 0,
                o.n_regions ? (int)d.chainable(0, shape[0], sw) : 0);
    mark();  // 2: <L,K> choice
    ClassMap by_shape = group_classes(o, shape, d, sw);
    const std::vector<uint32_t> reg_run = run_lengths(by_shape, o.n_regions, d, sw);
    mark();  // 3: classes, run lengths
    uint64_t best_cells = 0;
    std::string heaviest;  // the class with the most cells
    for (auto &kv : by_shape) {
        ShapeClass c = std::move(kv.second);
        finish_class(c, o, shape, reg_run, sw, flags, plan.n_reads);
        if (c.chain) join_chain_group(plan.chain_groups, c);
        plan.needs_redo = plan.needs_redo || c.f32_first;
        plan.max_h = std::max(plan.max_h, c.max_h);
        if (c.cells >= best_cells) {
            best_cells = c.cells;
            heaviest = c.name;
        }
        if (sw.trace)
            fprintf(stderr, "  class %-40s regions %6zu reads %8zu items %8zu cells %.3e max_h %u\n", c.name, c.regions.size(),
                    c.reads.size(), c.chain_items.size(), (double)c.cells, c.max_h);
        plan.classes.push_back(std::move(c));
    }
    mark();  // 4: work items per class
    account_swept(plan, o, shape, sw.trace != 0);
    for (auto &grp : plan.chain_groups) order_group(grp, o.read_off);
    plan.chain_groups = split_by_k_range(std::move(plan.chain_groups), o.read_off);
    plan.dominant = dominant_kernel(plan, std::move(heaviest));
    mark();  // 5: sorting, placement, ranges
    if (sw.trace)
        fprintf(stderr, "  plan phases (us): shapes %.0f, <L,K> %.0f, classes %.0f, items %.0f, order %.0f\n", marks[1] - marks[0],
                marks[2] - marks[1], marks[3] - marks[2], marks[4] - marks[3], marks[5] - marks[4]);
    return plan;
}

uint32_t num_launches(const BatchPlan &plan) {
    uint32_t n = 0;
    for (const auto &g : plan.chain_groups) n += g.items.empty() ? 0u : 1u;
    for (const auto &c : plan.classes)
        if (!c.chain || c.f32_first) n += 1u;  // per-read classes, and the f64 redo behind an f32 sweep
    return n;
}

}  // namespace phmm_plan
