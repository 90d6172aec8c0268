// Host side of the k-mer stage that phmm_assembly_kmers (phmm_asm.cpp) and phmm_assembly_graph (phmm_graph.cpp) share: the
// checks of the inputs both take, the staged inputs and the device-only workspace behind AsmParams.
#pragma once
#include <string>
#include <vector>

#include "phmm_asm_internal.hpp"
#include "phmm_host.hpp"
#include "phmm_staging.hpp"

namespace phmm {

struct AsmInputs {
    uint32_t n_regions;
    const uint32_t *region_ref_off;
    const uint8_t *ref_bases;
    const uint32_t *region_read_off, *read_off;
    const uint8_t *read_bases, *read_quals;
    const uint32_t *read_first, *read_len;
    uint32_t n_k;
    const uint32_t *k;
    uint32_t min_base_quality;
};

// What a caller says of its own arrays, checked where phmm_assembly_kmers always checked them: between the inputs' checks.
struct AsmOutputsGiven {
    bool pair_ok;            // its optional planes come together
    const char *pair_msg;
    bool region_arrays_ok;   // checked once n_regions > 0, with the region offsets
    bool ref_plane_ok;       // checked once there are reference bases, with ref_bases
    const char *ref_names;
    bool read_plane_ok;      // checked once there are read bases, with read_bases and read_quals
    const char *read_names;
};

// The batch as the checks leave it.
struct AsmBatch {
    uint32_t n_regions = 0, n_reads = 0, n_ref_bases = 0, n_read_bases = 0, n_slots = 0;
    bool long_sequence = false;
    std::vector<uint32_t> begin, len, read_region, region_plane_off, table_off;
};

struct AsmStaged {  // the inputs in the staging buffer
    StageSlot<uint32_t> ro, rr, po, to, rb, rl, rg;
    StageSlot<uint8_t> fb, db, dq;
};

struct AsmWorkspace {  // the device-only arrays in the handle's workspace
    StageSlot<uint64_t> fh, dh;
    StageSlot<uint16_t> re;
    StageSlot<uint32_t> ss, nr, st, sr, sb, si, fs, ds;
    StageSlot<uint8_t> fd, dd;
    StageSlot<unsigned long long> sc;
};

// PHMM_OK with `b` filled (b.n_regions == 0: nothing to do), or PHMM_ERR_INVALID_ARG with "<who>: <first offender>" in the handle.
int asm_check(phmm_handle *h, const char *who, const AsmInputs &in, const AsmOutputsGiven &given, AsmBatch &b);
AsmStaged asm_stage_inputs(phmm_host::StageLayout &L, const AsmInputs &in, const AsmBatch &b);
AsmWorkspace asm_plan_workspace(phmm_host::StageLayout &D, const AsmBatch &b, size_t nk);
// the handle's workspace with room for D; false with the error set
bool asm_reserve_workspace(phmm_handle *h, const phmm_host::StageLayout &D);
// everything of AsmParams but the results
void asm_bind(AsmParams &p, phmm_handle *h, const AsmInputs &in, const AsmBatch &b, const AsmStaged &s, const AsmWorkspace &w);

}  // namespace phmm
