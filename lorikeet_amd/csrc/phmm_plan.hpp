// The launch planner of the PairHMM engine: what a batch's kernels will be, worked out on the host from the batch's offset
// arrays alone.  plan_batch() makes no HIP runtime call and knows no handle; placing a finished plan in device memory
// is phmm_api.cpp's job (place_batch), and phmm_plan_describe is plan_batch() and nothing else.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "phmm_internal.hpp"

struct Switches;  // phmm_host.hpp

namespace phmm_plan {

constexpr size_t kLdsBytesPerCU = 160 * 1024;
constexpr uint32_t kNumSimd = 256 * 4;

// The flattened regions of a batch (include/phmm.h, phmm_batch_create): the planner reads the first four arrays.
struct BatchOffsets {
    uint32_t n_regions = 0;
    const uint32_t *region_read_off = nullptr, *region_hap_off = nullptr, *read_off = nullptr, *hap_off = nullptr;
    const uint64_t *out_off = nullptr;
};

struct ShapeClass {
    int L = 0, K = 0;  // L == 0 -> generic kernel
    std::vector<uint32_t> reads;  // global read indices (uploaded unless identity)
    bool identity = false;        // reads == 0..n-1
    uint32_t max_r = 0, max_h = 0, max_quads = 0;
    uint64_t cells = 0;
    // launch configuration
    uint32_t lds_rows = 8;
    int waves_per_block = phmm::MAX_WAVES_PER_BLOCK;
    size_t lds_bytes = 0;
    dim3 grid;
    // chained class: items are (region, haplotype group, run of reads) instead of single reads
    bool chain = false;
    std::vector<uint32_t> regions;  // member regions (chain classes)
    std::vector<phmm::ChainItem> chain_items;  // launched as part of its ChainGroup
    uint32_t cnd_select = 0;
    int streams = 1;  // chained classes: sub-runs swept side by side (phmm_chain_kernels.hip)
    bool f32_first = false;  // chained class at 16 lanes per pair of a PHMM_FLAG_F32_FIRST handle: f32 sweep, then the
                             // f64 per-read kernel over the reads it flagged (the per-read launch geometry is filled in too)
    // generic only
    std::vector<uint64_t> pair_first;
    uint32_t generic_blocks = 0;
    uint64_t generic_scratch_bytes = 0;  // (large: always an allocation of its own)
    char name[48] = {0};
};

// every chained f64 class of one lanes-per-pair value goes out in ONE launch (phmm_chain_kernels.hip)
struct ChainGroup {
    int L = 0;
    bool f32 = false;  // the f32 sweep of a PHMM_FLAG_F32_FIRST handle (the f64 per-read redo follows per class)
    int single_k = 0;  // the K all items share (per-K kernel), 0 = mixed (any-K kernel)
    std::vector<phmm::ChainItem> items;
};

struct BatchPlan {
    uint32_t n_regions = 0, n_reads = 0, n_haps = 0;
    uint64_t cells = 0, alg_bytes = 0;
    uint32_t max_h = 0;  // longest haplotype (sizes the scratch of phmm_rescue)
    std::vector<uint32_t> read_region;  // [n_reads]
    std::vector<ShapeClass> classes;
    std::vector<ChainGroup> chain_groups;  // in launch order
    bool needs_redo = false;  // f32-first mode: a class's f64 per-read kernel redoes the reads its f32 sweep flags ([n_reads] flags)
    std::string dominant;
    uint64_t pad_column_cells = 0, pad_slot_cells = 0;  // ... of which columns beyond a haplotype's end / haplotype slots left empty
    uint64_t swept_cells = 0;  // lane-cells the planned launches sweep: every row of every wave x 64 lanes x its K columns, padding
                               // columns, empty haplotype slots and all (phmm_batch_executed_cells)
};

// The plan of a batch whose offsets have passed phmm_host::validate_offsets.  `flags`: the handle's PHMM_FLAG_*; `gpu_sharers`:
// flows computing on the GPU at the same time.  Throws std::bad_alloc only.
BatchPlan plan_batch(const BatchOffsets &o, const Switches &sw, unsigned flags, uint32_t gpu_sharers);

uint32_t num_launches(const BatchPlan &plan);

}  // namespace phmm_plan
