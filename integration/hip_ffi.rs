//! `extern "C"` bindings of libphmm.so -- the MI355X-native PairHMM engine -- for Lorikeet.
//!
//! One declaration per export of `include/phmm.h`, same order, same argument order; nothing elided.
//! `tests/test_integration_artifacts.py` parses both files and fails when a name, an arity or a scalar width
//! differs.  This file is added to Lorikeet as `src/pair_hmm/hip_ffi.rs` by `integration/lorikeet-hip.patch`
//! (behind the cargo feature `hip`); the safe wrapper the PairHMM arm calls is `src/pair_hmm/hip_backend.rs`
//! of the same patch.
#![allow(non_camel_case_types, dead_code)]

use std::os::raw::{c_char, c_int, c_uint, c_void};

/// Opaque engine handle (`phmm_handle`).
#[repr(C)]
pub struct phmm_handle {
    _private: [u8; 0],
}
/// Opaque launch plan (`phmm_batch`).
#[repr(C)]
pub struct phmm_batch {
    _private: [u8; 0],
}

pub const PHMM_VERSION: c_int = 1;

pub const PHMM_FLAG_NO_TRISTATE: c_uint = 1;
pub const PHMM_FLAG_F32_FIRST: c_uint = 2;

pub const PHMM_OK: c_int = 0;
pub const PHMM_ERR_INVALID_ARG: c_int = 1;
pub const PHMM_ERR_NO_DEVICE: c_int = 2;
pub const PHMM_ERR_HIP: c_int = 3;
pub const PHMM_ERR_POSITIVE_RESULT: c_int = 4;
pub const PHMM_ERR_NOT_BOUND: c_int = 5;
pub const PHMM_ERR_NO_MEMORY: c_int = 6;
pub const PHMM_ERR_INTERNAL: c_int = 7;
pub const PHMM_ERR_CIGAR_CAPACITY: c_int = 8;
pub const PHMM_ERR_EVENT_CAPACITY: c_int = 9;

/// `overhang_strategy` of `phmm_sw_align` == gkl::smithwaterman::OverhangStrategy
pub const PHMM_SW_SOFTCLIP: c_int = 0;
pub const PHMM_SW_INDEL: c_int = 1;
pub const PHMM_SW_LEADING_INDEL: c_int = 2;
pub const PHMM_SW_IGNORE: c_int = 3;
/// `ref_index` value of `phmm_sw_align_indexed`: this alignment is skipped
pub const PHMM_SW_NO_REFERENCE: u32 = 0xffff_ffff;
/// `status` of `phmm_project_to_reference` (negative values: the read is one the reference panics on)
pub const PHMM_PROJECT_REALIGNED: c_int = 0;
pub const PHMM_PROJECT_UNCHANGED: c_int = 1;

/// `phmm_sw_parameters` == gkl::smithwaterman::Parameters::new(match, mismatch, gap open, gap extend)
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct phmm_sw_parameters {
    pub match_value: i32,
    pub mismatch_penalty: i32,
    pub gap_open_penalty: i32,
    pub gap_extend_penalty: i32,
}

/// `phmm_plan_info`: the launch plan of a batch, computed on the host alone (`phmm_plan_describe`)
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct phmm_plan_info {
    pub cells: u64,
    pub chain_cells: u64,
    pub chain_items: u64,
    pub n_launches: u32,
    pub n_chain_launches: u32,
    pub min_reads_per_run: u32,
    pub reserved: u32,
    pub dominant_kernel: [c_char; 64],
}

/// `flags` of `phmm_realign_config`: a region with exactly one haplotype is not realigned
/// (src/haplotype/haplotype_caller_engine.rs:1339-1345 returns before it gets there)
pub const PHMM_REGION_SKIP_SINGLE_ALLELE: c_uint = 1;

/// `phmm_allele_frequency`: allele kinds, per-event flags, per-allele flags
pub const PHMM_AF_KIND_PLAIN: c_int = 0;
pub const PHMM_AF_KIND_SPAN_DEL: c_int = 1;
pub const PHMM_AF_KIND_NON_REF: c_int = 2;
pub const PHMM_AF_CALLED: c_uint = 1;
pub const PHMM_AF_LOW_QUAL: c_uint = 2;
pub const PHMM_AF_MONOMORPHIC: c_uint = 4;
pub const PHMM_AF_TOO_MANY_ALLELES: c_uint = 8;
pub const PHMM_AF_NOT_CONVERGED: c_uint = 16;
pub const PHMM_AF_ALLELE_PLAUSIBLE: c_uint = 1;
pub const PHMM_AF_ALLELE_OUTPUT: c_uint = 2;
/// `phmm_assign_genotypes`: assignment methods, per-sample flags
pub const PHMM_GT_USE_PLS: c_uint = 0;
pub const PHMM_GT_USE_POSTERIORS: c_uint = 1;
pub const PHMM_GT_SAMPLE_UNINFORMATIVE: c_uint = 1;
pub const PHMM_GT_SAMPLE_NON_REF_BEST: c_uint = 2;
pub const PHMM_GT_SAMPLE_REF_ONLY: c_uint = 4;
/// `phmm_annotate_events`: per-event flags
pub const PHMM_ANN_NO_AD: c_uint = 1;
pub const PHMM_ANN_NO_QD: c_uint = 2;
pub const PHMM_ANN_QD_JITTER: c_uint = 4;
/// `phmm_discover_events`: limits per region, the event flag, the cached event types, region statuses
pub const PHMM_EVENTS_MAX_REF: c_uint = 16384;
pub const PHMM_EVENTS_MAX_HAPS: c_uint = 512;
pub const PHMM_EV_HAP_IN_TWO_ALLELES: c_uint = 1;
pub const PHMM_EV_TYPE_SNP: c_int = 1;
pub const PHMM_EV_TYPE_MNP: c_int = 2;
pub const PHMM_EV_TYPE_INDEL: c_int = 3;
pub const PHMM_EV_STATUS_BAD_OPERATOR: c_int = -1;
pub const PHMM_EV_STATUS_BLOCK: c_int = -2;
pub const PHMM_EV_STATUS_MERGE: c_int = -3;
pub const PHMM_EV_STATUS_CIGAR_OVERRUN: c_int = -4;
pub const PHMM_EV_STATUS_ALLELES: c_int = -5;
/// `phmm_activity_profile`: limits, window statuses
pub const PHMM_ACTIVITY_MAX_PLOIDY: c_uint = 64;
pub const PHMM_ACTIVITY_MAX_FILTER: c_uint = 65536;
pub const PHMM_ACT_STATUS_REF_SKIP: c_int = -1;
pub const PHMM_ACT_STATUS_CIGAR_OVERRUN: c_int = -2;
/// `phmm_finalize_reads`: the steps (`phmm_finalize_config::steps`) and the statuses of reads the reference would panic on
pub const PHMM_FIN_SOFT_CLIPS: c_uint = 1;
pub const PHMM_FIN_LOW_QUAL_ENDS: c_uint = 2;
pub const PHMM_FIN_ADAPTOR: c_uint = 4;
pub const PHMM_FIN_REGION: c_uint = 8;
pub const PHMM_FIN_PAIRS: c_uint = 16;
pub const PHMM_FIN_ALL: c_uint = 31;
pub const PHMM_FIN_STATUS_CIGAR: c_int = -1;
pub const PHMM_FIN_STATUS_CLIP_RANGE: c_int = -2;
pub const PHMM_FIN_STATUS_ARITHMETIC: c_int = -3;
pub const PHMM_FIN_STATUS_PAIR: c_int = -4;
pub const PHMM_FIN_STATUS_WORKSPACE: c_int = -5;
/// `phmm_phase_calls`: the flag that turns the reverse trim off, the region flag of a cleared mapping, the two phase groups
pub const PHMM_PH_NO_TRIM: c_uint = 1;
pub const PHMM_PH_ABORTED: c_uint = 1;
pub const PHMM_PH_GT_01: c_int = 0;
pub const PHMM_PH_GT_10: c_int = 1;
/// `phmm_assembly_kmers`: its limits, the verdicts per (k, region), the flags per (k, position)
pub const PHMM_ASM_MAX_K_VALUES: c_uint = 8;
pub const PHMM_ASM_MAX_K: c_uint = 255;
pub const PHMM_ASM_MAX_REF_BASES: c_uint = 16384;
pub const PHMM_ASM_MAX_READ_BASES: c_uint = 16384;
pub const PHMM_ASM_MAX_POSITIONS: c_uint = 536870912;
pub const PHMM_ASM_REF_SHORT: c_uint = 1;
pub const PHMM_ASM_REF_NON_UNIQUE: c_uint = 2;
pub const PHMM_ASM_LOW_COMPLEXITY: c_uint = 4;
pub const PHMM_ASM_KMER_NON_UNIQUE: c_uint = 1;
pub const PHMM_ASM_KMER_THREADED: c_uint = 2;
pub const PHMM_ASM_KMER_THREAD_START: c_uint = 4;
pub const PHMM_ASM_KMER_FIRST: c_uint = 8;
/// `phmm_assembly_graph`: its limits and the flags per vertex
pub const PHMM_GRAPH_MAX_SAMPLES: c_uint = 64;
pub const PHMM_GRAPH_MAX_PRUNING_SAMPLES: c_uint = 8;
pub const PHMM_GRAPH_VERTEX_TRACKED: c_uint = 1;
pub const PHMM_GRAPH_VERTEX_REF_SOURCE: c_uint = 2;
/// `phmm_assembly_prune`: the steps, the verdicts per graph, the bits per edge and per vertex
pub const PHMM_PRUNE_OP_CHAINS: c_uint = 1;
pub const PHMM_PRUNE_OP_CONNECT: c_uint = 2;
pub const PHMM_PRUNE_HAS_CYCLE: c_uint = 1;
pub const PHMM_PRUNE_NO_REF_ENDS: c_uint = 2;
pub const PHMM_PRUNE_ABSENT: c_uint = 1;
pub const PHMM_PRUNE_REMOVED_CHAINS: c_uint = 2;
pub const PHMM_PRUNE_REMOVED_CONNECT: c_uint = 4;
pub const PHMM_PRUNE_DANGLING_TAIL: c_uint = 8;
pub const PHMM_PRUNE_DANGLING_HEAD: c_uint = 16;
/// `phmm_assembly_recover`: the steps, an end's kind, and one status per exit of the reference's recovery
pub const PHMM_RECOVER_OP_TAILS: c_uint = 1;
pub const PHMM_RECOVER_OP_HEADS: c_uint = 2;
pub const PHMM_RECOVER_KIND_TAIL: c_uint = 0;
pub const PHMM_RECOVER_KIND_HEAD: c_uint = 1;
pub const PHMM_RECOVER_END_NO_PATH: c_uint = 0;
pub const PHMM_RECOVER_END_LOOP: c_uint = 1;
pub const PHMM_RECOVER_END_AT_REF_END: c_uint = 2;
pub const PHMM_RECOVER_END_TOO_SHORT: c_uint = 3;
pub const PHMM_RECOVER_END_CIGAR_NOT_OKAY: c_uint = 4;
pub const PHMM_RECOVER_END_TOO_FEW_MATCHING: c_uint = 5;
pub const PHMM_RECOVER_END_WHOLE_INSERTION: c_uint = 6;
pub const PHMM_RECOVER_END_TOO_MANY_MISMATCHES: c_uint = 7;
pub const PHMM_RECOVER_END_CANNOT_PUSH_REF: c_uint = 8;
pub const PHMM_RECOVER_END_CANNOT_EXTEND: c_uint = 9;
pub const PHMM_RECOVER_END_MERGED: c_uint = 10;
pub const PHMM_RECOVER_END_NO_MERGE_POINT: c_uint = 11;
pub const PHMM_RECOVER_END_REFERENCE_FAILS: c_uint = 12;
/// `phmm_assembly_seqgraph`: a graph's status
pub const PHMM_SEQ_OK: c_uint = 0;
pub const PHMM_SEQ_SKIPPED: c_uint = 1;
pub const PHMM_SEQ_REFERENCE_FAILS: c_uint = 2;
/// `phmm_assembly_best_paths`: a graph's status, the largest per-vertex total of multiplicities the log10 table serves, and the
/// `path_first_equal` of a path whose bytes are the region's reference (`u32::MAX`: the first of its bytes)
pub const PHMM_PATHS_OK: c_uint = 0;
pub const PHMM_PATHS_SKIPPED: c_uint = 1;
pub const PHMM_PATHS_NO_ENDS: c_uint = 2;
pub const PHMM_PATHS_NO_PATH: c_uint = 3;
pub const PHMM_PATHS_CYCLES_STAY: c_uint = 4;
pub const PHMM_PATHS_WEIGHT_RANGE: c_uint = 5;
pub const PHMM_PATHS_BUDGET: c_uint = 6;
pub const PHMM_PATHS_MAX_WEIGHT: c_uint = 1048576;
pub const PHMM_PATHS_EQUALS_REF: c_uint = 4294967294;
/// `phmm_trim_regions`: the two bits of `variation_present`, what became of an input haplotype (a rank otherwise), the statuses of
/// a region whose trimming panics in the reference (beside `PHMM_EV_STATUS_*` for a failed event map)
pub const PHMM_TRIM_VARIATION_SPAN: c_uint = 1;
pub const PHMM_TRIM_VARIATION_SET: c_uint = 2;
pub const PHMM_TRIM_FATE_DUPLICATE: c_int = -1;
pub const PHMM_TRIM_FATE_CUT_IN_DELETION: c_int = -2;
pub const PHMM_TRIM_FATE_EMPTY: c_int = -3;
pub const PHMM_TRIM_FATE_ALL_INSERTION: c_int = -4;
pub const PHMM_TRIM_FATE_NOT_TRIMMED: c_int = -5;
pub const PHMM_TRIM_STATUS_LOCATION: c_int = -16;
pub const PHMM_TRIM_STATUS_LENGTH: c_int = -17;
pub const PHMM_TRIM_STATUS_OPERATOR: c_int = -18;
pub const PHMM_TRIM_STATUS_NOT_FOUND: c_int = -19;
pub const PHMM_TRIM_STATUS_BUILDER: c_int = -20;
pub const PHMM_TRIM_STATUS_REF_ELIMINATED: c_int = -21;
pub const PHMM_TRIM_STATUS_REPEAT_SLICE: c_int = -22;
/// `phmm_assembly_regions`: the bits of `region_flags` and the statuses of a profile the reference panics on
pub const PHMM_REG_ACTIVE: c_uint = 1;
pub const PHMM_REG_FORCED: c_uint = 2;
pub const PHMM_REG_OVER_DEPTH: c_uint = 4;
pub const PHMM_REG_STATUS_MIN_REGION_SIZE: c_int = -1;
pub const PHMM_REG_STATUS_START_PAST_CONTIG: c_int = -2;

/// `phmm_finalize_config`: which steps of `finalize_regions` run, and their parameters
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct phmm_finalize_config {
    pub steps: u32,
    pub min_tail_quality: u8,
    pub dont_use_soft_clipped_bases: u8,
    pub half_of_pcr_snv_qual: u8,
    pub reserved: u8,
}

/// `phmm_recover_config`: which ends `phmm_assembly_recover` takes, and the reference's parameters of dangling-end recovery
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct phmm_recover_config {
    pub ops: u32,
    pub min_dangling_branch_length: i32,
    pub min_matching_bases: i32,
    pub max_mismatches_in_dangling_head: i32,
    pub num_pruning_samples: u32,
    pub sw_parameters: phmm_sw_parameters,
}

/// `phmm_realign_config`: what `realign_reads_to_their_best_haplotype` fixes at its call site
/// (src/reads/alignment_utils.rs:52-58, src/model/allele_likelihoods.rs:17)
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct phmm_realign_config {
    pub sw_parameters: phmm_sw_parameters,
    pub overhang_strategy: i32,
    pub flags: u32,
    pub informative_threshold: f64,
}

/// `phmm_engine_config`: the arguments of `PairHMMLikelihoodCalculationEngine::new`
/// (src/pair_hmm/pair_hmm_likelihood_calculation_engine.rs:129-141) the device needs.
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct phmm_engine_config {
    pub constant_gcp: u8,
    pub pcr_error_model: u8,
    pub base_quality_score_threshold: u8,
    pub dynamic_read_disqualification: u8,
    pub symmetrically_normalize_alleles_to_reference: u8,
    pub disable_cap_read_qualities_to_mapq: u8,
    pub reserved: [u8; 2],
    pub log10_global_read_mismapping_rate: f64,
    pub read_disqualification_scale: f64,
    pub expected_error_rate_per_base: f64,
}

extern "C" {
    pub fn phmm_device_count() -> c_int;
    pub fn phmm_create(device_id: c_int, flags: c_uint) -> *mut phmm_handle;
    pub fn phmm_destroy(h: *mut phmm_handle);
    pub fn phmm_last_error(h: *mut phmm_handle) -> *const c_char;

    pub fn phmm_compute(
        h: *mut phmm_handle,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        base_q: *const u8,
        ins_q: *const u8,
        del_q: *const u8,
        gcp: *const u8,
        hap_off: *const u32,
        hap_bases: *const u8,
        out_off: *const u64,
        out: *mut f64,
    ) -> c_int;

    pub fn phmm_submit(
        h: *mut phmm_handle,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        base_q: *const u8,
        ins_q: *const u8,
        del_q: *const u8,
        gcp: *const u8,
        hap_off: *const u32,
        hap_bases: *const u8,
        out_off: *const u64,
        out: *mut f64,
        ticket: *mut u64,
    ) -> c_int;
    pub fn phmm_wait(h: *mut phmm_handle, ticket: u64) -> c_int;
    pub fn phmm_submit_stats(h: *mut phmm_handle, n_flushes: *mut u64, n_submissions: *mut u64);

    pub fn phmm_assign_regions(
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        hap_off: *const u32,
        n_parts: u32,
        part_of_region: *mut u32,
    ) -> c_int;
    pub fn phmm_split_regions(
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        hap_off: *const u32,
        n_parts: u32,
        first_region: *mut u32,
    ) -> c_int;
    pub fn phmm_compute_multi(
        handles: *const *mut phmm_handle,
        n_handles: u32,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        base_q: *const u8,
        ins_q: *const u8,
        del_q: *const u8,
        gcp: *const u8,
        hap_off: *const u32,
        hap_bases: *const u8,
        out_off: *const u64,
        out: *mut f64,
    ) -> c_int;

    pub fn phmm_batch_create(
        h: *mut phmm_handle,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        hap_off: *const u32,
        out_off: *const u64,
    ) -> *mut phmm_batch;
    pub fn phmm_batch_destroy(b: *mut phmm_batch);
    pub fn phmm_batch_bind_device(
        b: *mut phmm_batch,
        d_read_bases: *const u8,
        d_base_q: *const u8,
        d_ins_q: *const u8,
        d_del_q: *const u8,
        d_gcp: *const u8,
        d_hap_bases: *const u8,
        d_out: *mut f64,
    ) -> c_int;
    pub fn phmm_batch_upload(
        b: *mut phmm_batch,
        read_bases: *const u8,
        base_q: *const u8,
        ins_q: *const u8,
        del_q: *const u8,
        gcp: *const u8,
        hap_bases: *const u8,
    ) -> c_int;
    pub fn phmm_batch_launch(b: *mut phmm_batch, stream: *mut c_void) -> c_int;
    pub fn phmm_batch_download(b: *mut phmm_batch, out: *mut f64) -> c_int;
    pub fn phmm_batch_status(b: *mut phmm_batch) -> c_int;
    pub fn phmm_batch_cells(b: *const phmm_batch) -> u64;
    pub fn phmm_batch_algorithmic_bytes(b: *const phmm_batch) -> u64;
    pub fn phmm_batch_num_launches(b: *const phmm_batch) -> u32;
    pub fn phmm_batch_executed_cells(b: *const phmm_batch) -> u64;
    pub fn phmm_batch_dominant_kernel(b: *const phmm_batch) -> *const c_char;
    pub fn phmm_plan_describe(
        flags: c_uint,
        concurrent_callers: u32,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        hap_off: *const u32,
        info: *mut phmm_plan_info,
    ) -> c_int;

    pub fn phmm_engine_compute(
        h: *mut phmm_handle,
        cfg: *const phmm_engine_config,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        base_q: *const u8,
        ins_q: *const u8,
        del_q: *const u8,
        mapq: *const u8,
        hap_off: *const u32,
        hap_bases: *const u8,
        region_ref_hap: *const i32,
        out_off: *const u64,
        out: *mut f64,
        keep: *mut u8,
    ) -> c_int;
    pub fn phmm_engine_submit(
        h: *mut phmm_handle,
        cfg: *const phmm_engine_config,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        base_q: *const u8,
        ins_q: *const u8,
        del_q: *const u8,
        mapq: *const u8,
        hap_off: *const u32,
        hap_bases: *const u8,
        region_ref_hap: *const i32,
        out_off: *const u64,
        out: *mut f64,
        keep: *mut u8,
        ticket: *mut u64,
    ) -> c_int;

    pub fn phmm_engine_compute_multi(
        handles: *const *mut phmm_handle,
        n_handles: u32,
        cfg: *const phmm_engine_config,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        base_q: *const u8,
        ins_q: *const u8,
        del_q: *const u8,
        mapq: *const u8,
        hap_off: *const u32,
        hap_bases: *const u8,
        region_ref_hap: *const i32,
        out_off: *const u64,
        out: *mut f64,
        keep: *mut u8,
    ) -> c_int;

    pub fn phmm_sw_align(
        h: *mut phmm_handle,
        n_alignments: u32,
        ref_off: *const u32,
        ref_bases: *const u8,
        alt_off: *const u32,
        alt_bases: *const u8,
        params: *const phmm_sw_parameters,
        overhang_strategy: c_int,
        cigar_off: *const u64,
        cigar: *mut u32,
        n_cigar: *mut u32,
        alignment_offset: *mut i32,
    ) -> c_int;

    pub fn phmm_sw_align_indexed(
        h: *mut phmm_handle,
        n_references: u32,
        ref_off: *const u32,
        ref_bases: *const u8,
        n_alignments: u32,
        ref_index: *const u32,
        alt_off: *const u32,
        alt_bases: *const u8,
        params: *const phmm_sw_parameters,
        overhang_strategy: c_int,
        cigar_off: *const u64,
        cigar: *mut u32,
        n_cigar: *mut u32,
        alignment_offset: *mut i32,
    ) -> c_int;

    pub fn phmm_best_alleles(
        h: *mut phmm_handle,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        out_off: *const u64,
        likelihoods: *const f64,
        keep: *const u8,
        hap_priority: *const i32,
        informative_threshold: f64,
        best_allele: *mut i32,
        likelihood: *mut f64,
        confidence: *mut f64,
    ) -> c_int;

    pub fn phmm_realign_to_best(
        h: *mut phmm_handle,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        hap_off: *const u32,
        hap_bases: *const u8,
        out_off: *const u64,
        likelihoods: *const f64,
        keep: *const u8,
        hap_priority: *const i32,
        informative_threshold: f64,
        params: *const phmm_sw_parameters,
        overhang_strategy: c_int,
        cigar_off: *const u64,
        cigar: *mut u32,
        n_cigar: *mut u32,
        alignment_offset: *mut i32,
        best_allele: *mut i32,
        likelihood: *mut f64,
        confidence: *mut f64,
    ) -> c_int;

    pub fn phmm_project_to_reference(
        h: *mut phmm_handle,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        hap_off: *const u32,
        hap_bases: *const u8,
        region_ref_hap: *const i32,
        region_reference_start: *const u64,
        hap_cigar_off: *const u32,
        hap_cigar: *const u32,
        hap_start_wrt_ref: *const u32,
        best_allele: *const i32,
        sw_cigar_off: *const u64,
        sw_cigar: *const u32,
        n_sw_cigar: *const u32,
        sw_offset: *const i32,
        orig_cigar_off: *const u32,
        orig_cigar: *const u32,
        out_cigar_off: *const u64,
        out_cigar: *mut u32,
        n_out_cigar: *mut u32,
        new_pos: *mut i64,
        status: *mut i32,
    ) -> c_int;

    pub fn phmm_realign_reads(
        h: *mut phmm_handle,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        hap_off: *const u32,
        hap_bases: *const u8,
        out_off: *const u64,
        likelihoods: *const f64,
        keep: *const u8,
        hap_priority: *const i32,
        informative_threshold: f64,
        params: *const phmm_sw_parameters,
        overhang_strategy: c_int,
        region_ref_hap: *const i32,
        region_reference_start: *const u64,
        hap_cigar_off: *const u32,
        hap_cigar: *const u32,
        hap_start_wrt_ref: *const u32,
        orig_cigar_off: *const u32,
        orig_cigar: *const u32,
        out_cigar_off: *const u64,
        out_cigar: *mut u32,
        n_out_cigar: *mut u32,
        new_pos: *mut i64,
        status: *mut i32,
        best_allele: *mut i32,
        likelihood: *mut f64,
        confidence: *mut f64,
    ) -> c_int;

    pub fn phmm_region_compute(
        h: *mut phmm_handle,
        cfg: *const phmm_engine_config,
        rcfg: *const phmm_realign_config,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        base_q: *const u8,
        ins_q: *const u8,
        del_q: *const u8,
        mapq: *const u8,
        read_soft_clip: *const u32,
        hap_off: *const u32,
        hap_bases: *const u8,
        region_ref_hap: *const i32,
        out_off: *const u64,
        hap_priority: *const i32,
        region_reference_start: *const u64,
        hap_cigar_off: *const u32,
        hap_cigar: *const u32,
        hap_start_wrt_ref: *const u32,
        orig_cigar_off: *const u32,
        orig_cigar: *const u32,
        out_cigar_off: *const u64,
        out: *mut f64,
        keep: *mut u8,
        best_allele: *mut i32,
        likelihood: *mut f64,
        confidence: *mut f64,
        out_cigar: *mut u32,
        n_out_cigar: *mut u32,
        new_pos: *mut i64,
        status: *mut i32,
    ) -> c_int;

    pub fn phmm_region_submit(
        h: *mut phmm_handle,
        cfg: *const phmm_engine_config,
        rcfg: *const phmm_realign_config,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        base_q: *const u8,
        ins_q: *const u8,
        del_q: *const u8,
        mapq: *const u8,
        read_soft_clip: *const u32,
        hap_off: *const u32,
        hap_bases: *const u8,
        region_ref_hap: *const i32,
        out_off: *const u64,
        hap_priority: *const i32,
        region_reference_start: *const u64,
        hap_cigar_off: *const u32,
        hap_cigar: *const u32,
        hap_start_wrt_ref: *const u32,
        orig_cigar_off: *const u32,
        orig_cigar: *const u32,
        out_cigar_off: *const u64,
        out: *mut f64,
        keep: *mut u8,
        best_allele: *mut i32,
        likelihood: *mut f64,
        confidence: *mut f64,
        out_cigar: *mut u32,
        n_out_cigar: *mut u32,
        new_pos: *mut i64,
        status: *mut i32,
        ticket: *mut u64,
    ) -> c_int;

    pub fn phmm_region_compute_multi(
        handles: *const *mut phmm_handle,
        n_handles: u32,
        cfg: *const phmm_engine_config,
        rcfg: *const phmm_realign_config,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        base_q: *const u8,
        ins_q: *const u8,
        del_q: *const u8,
        mapq: *const u8,
        read_soft_clip: *const u32,
        hap_off: *const u32,
        hap_bases: *const u8,
        region_ref_hap: *const i32,
        out_off: *const u64,
        hap_priority: *const i32,
        region_reference_start: *const u64,
        hap_cigar_off: *const u32,
        hap_cigar: *const u32,
        hap_start_wrt_ref: *const u32,
        orig_cigar_off: *const u32,
        orig_cigar: *const u32,
        out_cigar_off: *const u64,
        out: *mut f64,
        keep: *mut u8,
        best_allele: *mut i32,
        likelihood: *mut f64,
        confidence: *mut f64,
        out_cigar: *mut u32,
        n_out_cigar: *mut u32,
        new_pos: *mut i64,
        status: *mut i32,
    ) -> c_int;

    pub fn phmm_calculate_cigar(
        h: *mut phmm_handle,
        n: u32,
        ref_off: *const u32,
        ref_bases: *const u8,
        alt_off: *const u32,
        alt_bases: *const u8,
        params: *const phmm_sw_parameters,
        overhang_strategy: c_int,
        cigar_off: *const u64,
        cigar: *mut u32,
        n_cigar: *mut u32,
        status: *mut i32,
    ) -> c_int;

    /// genotyping_engine.assign_genotype_likelihoods per event (haplotype_caller_engine.rs:1379): marginalized likelihoods,
    /// the overlapping reads of each sample, GLs and PLs for every genotype in the reference's index order
    pub fn phmm_genotype_count(ploidy: u32, n_alleles: u32) -> u32;
    pub fn phmm_genotype_likelihoods(
        h: *mut phmm_handle,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        out_off: *const u64,
        likelihoods: *const f64,
        keep: *const u8,
        read_sample: *const u32,
        read_start: *const i64,
        read_end: *const i64,
        n_samples: u32,
        ploidy: u32,
        n_events: u32,
        event_region: *const u32,
        event_allele_off: *const u32,
        event_start: *const i64,
        event_end: *const i64,
        event_hap_allele: *const i32,
        gl_off: *const u64,
        gl: *mut f64,
        pl: *mut i32,
        n_evidence: *mut u32,
    ) -> c_int;
    /// GenotypingEngine::calculate_genotypes' arithmetic per event (genotyping_engine.rs:80-197): the EM allele-frequency
    /// calculation on the PLs above, P(no variant), P(allele absent), MLE counts, the output subset and QUAL
    pub fn phmm_allele_frequency(
        h: *mut phmm_handle,
        n_events: u32,
        n_samples: u32,
        ploidy: u32,
        event_allele_off: *const u32,
        allele_length: *const u32,
        allele_kind: *const u8,
        pl_off: *const u64,
        pl: *const i32,
        ref_pseudo_count: f64,
        snp_pseudo_count: f64,
        indel_pseudo_count: f64,
        stand_min_conf: f64,
        log10_p_no_variant: *mut f64,
        log10_p_variant_present: *mut f64,
        log10_p_absent: *mut f64,
        mle_count: *mut i64,
        allele_flags: *mut u8,
        qual: *mut f64,
        flags: *mut u32,
        iterations: *mut u32,
    ) -> c_int;
    /// AlleleSubsettingUtils::subset_alleles and VariantContext::make_genotype_call per event and sample
    /// (genotyping_engine.rs:199-235): the subsetted PLs, GT, GQ, the sample_called flags of phmm_annotate_events, and with
    /// the posterior method GP, PG and the QUAL update
    pub fn phmm_assign_genotypes(
        h: *mut phmm_handle,
        n_events: u32,
        n_samples: u32,
        ploidy: u32,
        event_allele_off: *const u32,
        allele_length: *const u32,
        allele_kind: *const u8,
        pl_off: *const u64,
        pl: *const i32,
        call_allele_off: *const u32,
        call_allele: *const u32,
        method: u32,
        log10_snp_het: f64,
        log10_indel_het: f64,
        site_monomorphic: *const u8,
        sub_pl_off: *const u64,
        sub_pl: *mut i32,
        gt: *mut i32,
        gq: *mut i32,
        log10_gq: *mut f64,
        sample_called: *mut u8,
        sample_flags: *mut u8,
        gp: *mut f64,
        pg: *mut f64,
        log10_p_error_posterior: *mut f64,
    ) -> c_int;
    /// the marginal onto the alleles of the call and VariantAnnotationEngine::annotate_context over it
    /// (haplotype_caller_genotyping_engine.rs:330-393, variant_annotation.rs:93-405): AD, DP, AF, AC per sample, DP, QD, MQ, BQ per event
    pub fn phmm_annotate_events(
        h: *mut phmm_handle,
        n_regions: u32,
        region_read_off: *const u32,
        region_hap_off: *const u32,
        out_off: *const u64,
        likelihoods: *const f64,
        keep: *const u8,
        read_sample: *const u32,
        read_start: *const i64,
        read_end: *const i64,
        mapq: *const u8,
        n_samples: u32,
        n_events: u32,
        event_region: *const u32,
        event_allele_off: *const u32,
        event_start: *const i64,
        event_end: *const i64,
        event_hap_allele: *const i32,
        call_allele_off: *const u32,
        call_allele: *const u32,
        read_off: *const u32,
        base_q: *const u8,
        out_cigar_off: *const u64,
        out_cigar: *const u32,
        n_out_cigar: *const u32,
        read_soft_start: *const i64,
        event_pos: *const i64,
        sample_called: *const u8,
        log10_p_error: *const f64,
        n_filtered: *const u32,
        ad: *mut i32,
        dp: *mut i32,
        af: *mut f64,
        ac: *mut u32,
        mq: *mut u8,
        bq: *mut u8,
        info_dp: *mut i32,
        qd_depth: *mut i32,
        qd: *mut f64,
        flags: *mut u32,
    ) -> c_int;
    /// the head of assign_genotype_likelihoods (haplotype_caller_genotyping_engine.rs:125-229): the haplotypes' event maps,
    /// the loci, the merged alleles and the haplotype -> allele map of every event, dense, as the four calls above take them
    pub fn phmm_discover_events(
        h: *mut phmm_handle,
        n_regions: u32,
        region_ref_off: *const u32,
        ref_bases: *const u8,
        region_ref_start: *const u64,
        region_window_start: *const u64,
        region_window_end: *const u64,
        region_contig_length: *const u64,
        region_hap_off: *const u32,
        hap_off: *const u32,
        hap_bases: *const u8,
        hap_cigar_off: *const u32,
        hap_cigar: *const u32,
        hap_start_wrt_ref: *const u32,
        max_mnp_distance: u32,
        include_spanning_events: c_int,
        overlap_margin: u32,
        capacity: *const u32,
        required: *mut u32,
        region_event_off: *mut u32,
        region_status: *mut i32,
        event_region: *mut u32,
        event_allele_off: *mut u32,
        event_start: *mut i64,
        event_end: *mut i64,
        event_loc: *mut i64,
        vc_start: *mut i64,
        vc_end: *mut i64,
        event_flags: *mut u32,
        event_hap_allele: *mut i32,
        allele_length: *mut u32,
        allele_kind: *mut u8,
        allele_bases_off: *mut u32,
        allele_bases: *mut u8,
        hap_event_off: *mut u32,
        hap_event_start: *mut i64,
        hap_event_end: *mut i64,
        hap_event_ref_length: *mut u32,
        hap_event_alt_off: *mut u32,
        hap_event_alt: *mut u8,
        hap_event_type: *mut u32,
    ) -> c_int;
    /// the activity profile (haplotype_caller_engine.rs:627-1107, band_pass_activity_profile.rs): per (window, sample, position)
    /// the RefVsAnyResult, per position the soft-clip average and is_active_prob (f32), per profile the band-passed state list
    /// (f32); every output but window_status may be null
    pub fn phmm_activity_profile(
        h: *mut phmm_handle,
        n_windows: u32,
        n_samples: u32,
        ploidy: u32,
        min_base_quality: u32,
        ref_pseudo_count: f64,
        snp_pseudo_count: f64,
        indel_pseudo_count: f64,
        stand_min_conf: f64,
        max_prob_propagation: u32,
        max_filter_size: u32,
        sigma: f64,
        adaptive_filter_size: c_int,
        profile_size: u32,
        window_start: *const u64,
        window_len: *const u32,
        window_contig_length: *const u64,
        window_ref_off: *const u32,
        ref_bases: *const u8,
        group_read_off: *const u32,
        read_pos: *const i64,
        read_cigar_off: *const u32,
        read_cigar: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        read_quals: *const u8,
        window_status: *mut i32,
        read_counts: *mut u32,
        ref_depth: *mut u32,
        non_ref_depth: *mut u32,
        gl: *mut f64,
        pl: *mut i32,
        soft_clip_mean: *mut f64,
        soft_clip_count: *mut u32,
        qual: *mut f64,
        af_flags: *mut u32,
        is_active_prob: *mut c_void,
        filter_size: *mut u32,
        profile_prob: *mut c_void,
        profile_len: *mut u32,
    ) -> c_int;
    /// (parity tests: the host-made Gaussian kernel and the per-(is_alt, quality) addends of the activity profile)
    pub fn phmm_activity_band_kernel(max_filter_size: u32, sigma: f64, adaptive_filter_size: c_int, filter_size: *mut u32, kernel: *mut f64) -> c_int;
    pub fn phmm_activity_term_table(ploidy: u32, term: *mut f64) -> c_int;
    /// a region's reads finalized (assembly_based_caller_utils.rs:97-172, :263-289; assembly_region.rs:341-352): soft clips,
    /// low-quality tails, adaptor, the clip to the padded span, the filter, the qualities of overlapping mates; every output
    /// but read_status may be null.  `cfg` points to a `phmm_finalize_config`, `read_flags` to `[u16; n_reads]`
    pub fn phmm_finalize_reads(
        h: *mut phmm_handle,
        cfg: *const c_void,
        n_groups: u32,
        group_read_off: *const u32,
        group_span_start: *const u64,
        group_span_end: *const u64,
        read_pos: *const i64,
        read_flags: *const c_void,
        read_mapq: *const u8,
        read_mpos: *const i64,
        read_isize: *const i64,
        read_cigar_off: *const u32,
        read_cigar: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        read_quals: *const u8,
        mate_index: *const i32,
        out_cigar_off: *const u64,
        read_status: *mut i32,
        keep: *mut u8,
        new_pos: *mut i64,
        out_unmapped: *mut u8,
        clip_first: *mut u32,
        clip_len: *mut u32,
        out_cigar: *mut u32,
        n_out_cigar: *mut u32,
        unclipped_len: *mut u32,
        lead_soft: *mut u32,
        trail_soft: *mut u32,
        out_quals: *mut u8,
    ) -> c_int;
    /// the called events of many regions reverse-trimmed and phased (haplotype_caller_genotyping_engine.rs:394-405, :451-489;
    /// variant_context_utils.rs:956-1108; assembly_based_caller_utils.rs:975-1348) on the arrays `phmm_discover_events` writes and
    /// the call lists and GT of `phmm_annotate_events` / `phmm_assign_genotypes`; `gt`, `is_phased`, `gt_phased` are null
    /// together, `hap_in_call` may be null
    pub fn phmm_phase_calls(
        h: *mut phmm_handle,
        n_regions: u32,
        region_event_off: *const u32,
        region_hap_off: *const u32,
        event_allele_off: *const u32,
        event_hap_allele: *const i32,
        vc_start: *const i64,
        allele_length: *const u32,
        allele_kind: *const u8,
        allele_bases_off: *const u32,
        allele_bases: *const u8,
        hap_event_off: *const u32,
        hap_event_start: *const i64,
        hap_event_alt_off: *const u32,
        hap_event_alt: *const u8,
        call_allele_off: *const u32,
        call_allele: *const u32,
        n_samples: u32,
        ploidy: u32,
        gt: *const i32,
        flags: u32,
        call_rev_trim: *mut u32,
        call_end: *mut i64,
        phase_n_haps: *mut u32,
        hap_in_call: *mut u8,
        phase_group: *mut i32,
        phase_gt: *mut u8,
        phase_leader: *mut i32,
        phase_set: *mut i64,
        region_alt_haps: *mut u32,
        region_phase_flags: *mut u32,
        is_phased: *mut u8,
        gt_phased: *mut i32,
    ) -> c_int;
    /// what the read-threading assembler decides from k-mers alone, for many regions and several k (read_threading_graph.rs:111-187,
    /// :341-403, :484-639; read_threading_assembler.rs:935-956): verdicts and counts per (k, region), flags and dense ids per
    /// (k, position); `read_first` / `read_len` are null together, and so are the two id planes
    pub fn phmm_assembly_kmers(
        h: *mut phmm_handle,
        n_regions: u32,
        region_ref_off: *const u32,
        ref_bases: *const u8,
        region_read_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        read_quals: *const u8,
        read_first: *const u32,
        read_len: *const u32,
        n_k: u32,
        k: *const u32,
        min_base_quality: u32,
        flags: *mut u32,
        n_sequences: *mut u32,
        n_non_unique: *mut u32,
        n_tracked: *mut u32,
        n_distinct: *mut u32,
        ref_kmer_flags: *mut u8,
        read_kmer_flags: *mut u8,
        ref_kmer_id: *mut u32,
        read_kmer_id: *mut u32,
    ) -> c_int;
    /// the raw read-threading graph per (k, region) as build_graph_if_necessary leaves it (read_threading_graph.rs:417-477, :484-769;
    /// multi_sample_edge.rs), default modes: vertices in NodeIndex order, edges in EdgeIndex order with both multiplicities, the
    /// reference path, and on request the vertex of every visited position; `capacity` / `required`: vertices, edges, ref_path
    /// entries; `read_sample`, `read_first` / `read_len` and the two vertex planes may be null
    pub fn phmm_assembly_graph(
        h: *mut phmm_handle,
        n_regions: u32,
        region_ref_off: *const u32,
        ref_bases: *const u8,
        region_read_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        read_quals: *const u8,
        read_first: *const u32,
        read_len: *const u32,
        read_sample: *const u32,
        n_k: u32,
        k: *const u32,
        min_base_quality: u32,
        num_pruning_samples: u32,
        capacity: *const u32,
        required: *mut u32,
        flags: *mut u32,
        n_vertices: *mut u32,
        n_edges: *mut u32,
        n_ref_path: *mut u32,
        vertex_off: *mut u32,
        edge_off: *mut u32,
        ref_path_off: *mut u32,
        vertex_seq: *mut u32,
        vertex_pos: *mut u32,
        vertex_flags: *mut u8,
        edge_src: *mut u32,
        edge_dst: *mut u32,
        edge_is_ref: *mut u8,
        edge_multiplicity: *mut u32,
        edge_pruning_multiplicity: *mut u32,
        ref_path: *mut u32,
        ref_vertex: *mut u32,
        read_vertex: *mut u32,
    ) -> c_int;
    /// what create_graph does to the raw graph before it looks for paths (read_threading_assembler.rs:1041-1073, :1118-1136), for
    /// many graphs: low-weight chains (chain_pruner.rs:39-118, low_weight_chain_pruner.rs:24-36), orphans, the cycle verdict, the
    /// reference ends, the dangling ends and remove_paths_not_connected_to_ref (base_graph.rs:339-428, :615-656); the two
    /// `absent` masks are null together
    pub fn phmm_assembly_prune(
        h: *mut phmm_handle,
        n_graphs: u32,
        vertex_off: *const u32,
        edge_off: *const u32,
        edge_src: *const u32,
        edge_dst: *const u32,
        edge_is_ref: *const u8,
        edge_pruning_multiplicity: *const u32,
        vertex_absent: *const u8,
        edge_absent: *const u8,
        ops: u32,
        prune_factor: *const u32,
        graph_flags: *mut u32,
        n_chains: *mut u32,
        n_chains_removed: *mut u32,
        n_vertices_left: *mut u32,
        n_edges_left: *mut u32,
        ref_source: *mut u32,
        ref_sink: *mut u32,
        edge_chain: *mut u32,
        edge_state: *mut u8,
        vertex_state: *mut u8,
    ) -> c_int;
    /// dangling-end recovery (read_threading_graph.rs:779-1766): recover_dangling_tails, then recover_dangling_heads, for many
    /// graphs, every end of a graph after the one before it; `cfg` points to a `phmm_recover_config`; the two `absent` masks are
    /// null together, `graph_flags` may be null; `capacity` / `required` count ends, new edges and new vertices
    pub fn phmm_assembly_recover(
        h: *mut phmm_handle,
        cfg: *const c_void,
        n_regions: u32,
        region_ref_off: *const u32,
        ref_bases: *const u8,
        region_read_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        read_first: *const u32,
        read_len: *const u32,
        n_k: u32,
        k: *const u32,
        vertex_off: *const u32,
        edge_off: *const u32,
        vertex_seq: *const u32,
        vertex_pos: *const u32,
        edge_src: *const u32,
        edge_dst: *const u32,
        edge_is_ref: *const u8,
        edge_multiplicity: *const u32,
        edge_pruning_multiplicity: *const u32,
        vertex_absent: *const u8,
        edge_absent: *const u8,
        graph_flags: *const u32,
        prune_factor: *const u32,
        capacity: *const u32,
        required: *mut u32,
        n_tails: *mut u32,
        n_tails_recovered: *mut u32,
        n_heads: *mut u32,
        n_heads_recovered: *mut u32,
        n_new_edges: *mut u32,
        n_new_vertices: *mut u32,
        n_rounds: *mut u32,
        end_off: *mut u32,
        new_edge_off: *mut u32,
        new_vertex_off: *mut u32,
        end_vertex: *mut u32,
        end_kind: *mut u32,
        end_status: *mut u32,
        end_alt_len: *mut u32,
        end_ref_len: *mut u32,
        end_n_cigar: *mut u32,
        end_cigar: *mut u32,
        end_edge: *mut u32,
        new_edge_src: *mut u32,
        new_edge_dst: *mut u32,
        new_edge_multiplicity: *mut u32,
        new_edge_pruning_multiplicity: *mut u32,
        new_vertex_kmer: *mut u8,
        edge_removed: *mut u8,
    ) -> c_int;
    /// the zipped sequence graph (base_graph.rs:54-84, 716-793, seq_graph.rs:189-369): to_sequence_graph, clean_non_ref_paths, the first
    /// zip_linear_chains, the orphans and the vertices the reference source neither reaches nor is reached from, for many graphs;
    /// `new_vertex_off` / `new_vertex_kmer` are null together, as are the two `absent` masks; `graph_flags` and `vertex_to_seq` may be
    /// null; `capacity` / `required` count sequence vertices, sequence edges and sequence bytes
    pub fn phmm_assembly_seqgraph(
        h: *mut phmm_handle,
        n_regions: u32,
        region_ref_off: *const u32,
        ref_bases: *const u8,
        region_read_off: *const u32,
        read_off: *const u32,
        read_bases: *const u8,
        read_first: *const u32,
        read_len: *const u32,
        n_k: u32,
        k: *const u32,
        vertex_off: *const u32,
        edge_off: *const u32,
        vertex_seq: *const u32,
        vertex_pos: *const u32,
        edge_src: *const u32,
        edge_dst: *const u32,
        edge_is_ref: *const u8,
        edge_multiplicity: *const u32,
        new_vertex_off: *const u32,
        new_vertex_kmer: *const u8,
        vertex_absent: *const u8,
        edge_absent: *const u8,
        graph_flags: *const u32,
        capacity: *const u32,
        required: *mut u32,
        seq_status: *mut u32,
        n_seq_vertices: *mut u32,
        n_seq_edges: *mut u32,
        n_seq_bases: *mut u32,
        n_chains_zipped: *mut u32,
        n_removed_clean: *mut u32,
        n_removed_unconnected: *mut u32,
        seq_ref_source: *mut u32,
        seq_ref_sink: *mut u32,
        seq_vertex_off: *mut u32,
        seq_edge_off: *mut u32,
        seq_base_off: *mut u32,
        seq_vertex_base_off: *mut u32,
        seq_vertex_first: *mut u32,
        seq_vertex_n_merged: *mut u32,
        seq_edge_src: *mut u32,
        seq_edge_dst: *mut u32,
        seq_edge_is_ref: *mut u8,
        seq_edge_multiplicity: *mut u32,
        seq_bases: *mut u8,
        vertex_to_seq: *mut u32,
    ) -> c_int;
    /// the k best haplotype paths of many sequence graphs (k_best_haplotype_finder.rs:71-182, graph_based_k_best_haplotype_finder.rs:64-132,
    /// k_best_haplotype.rs:86-112, path.rs:234-267): the cycle removal as written, the best-first search, the paths' bases and the
    /// duplicate marks; `seq_status`, `vertex_role` (then `graph_source` / `graph_sink` too), the region arguments, `path_first_equal`,
    /// `edge_removed` and `vertex_removed` may be null / 0; `capacity` / `required` count paths, path edges and haplotype bytes
    pub fn phmm_assembly_best_paths(
        h: *mut phmm_handle,
        n_graphs: u32,
        seq_vertex_off: *const u32,
        seq_edge_off: *const u32,
        seq_base_off: *const u32,
        seq_vertex_base_off: *const u32,
        seq_edge_src: *const u32,
        seq_edge_dst: *const u32,
        seq_edge_is_ref: *const u8,
        seq_edge_multiplicity: *const u32,
        seq_bases: *const u8,
        seq_status: *const u32,
        graph_source: *const u32,
        graph_sink: *const u32,
        vertex_role: *const u8,
        max_paths: u32,
        max_nodes_per_graph: u32,
        n_regions: u32,
        n_k: u32,
        region_ref_off: *const u32,
        ref_bases: *const u8,
        capacity: *const u32,
        required: *mut u32,
        paths_status: *mut u32,
        n_paths: *mut u32,
        n_popped: *mut u32,
        n_cycle_edges_removed: *mut u32,
        n_cycle_vertices_removed: *mut u32,
        path_off: *mut u32,
        path_edge_off: *mut u32,
        hap_base_off: *mut u32,
        path_score: *mut f64,
        path_is_ref: *mut u8,
        path_n_edges: *mut u32,
        hap_off: *mut u32,
        path_first_equal: *mut u32,
        path_edges: *mut u32,
        hap_bases: *mut u8,
        edge_removed: *mut u8,
        vertex_removed: *mut u8,
    ) -> c_int;
    /// what call_region does with the assembler's haplotypes before a likelihood is computed (haplotype_caller_engine.rs:1194-1243):
    /// the trimmer's spans, every haplotype cut to the padded span, duplicates folded, the rest in the BTreeMap's order, dense;
    /// `padding`: SNP, indel, STR padding and max_extension_into_region_padding
    pub fn phmm_trim_regions(
        h: *mut phmm_handle,
        n_regions: u32,
        region_ref_off: *const u32,
        ref_bases: *const u8,
        region_ref_start: *const u64,
        region_active_start: *const u64,
        region_active_end: *const u64,
        region_padded_start: *const u64,
        region_padded_end: *const u64,
        region_hap_off: *const u32,
        hap_off: *const u32,
        hap_bases: *const u8,
        hap_cigar_off: *const u32,
        hap_cigar: *const u32,
        hap_start_wrt_ref: *const u32,
        hap_loc_start: *const u64,
        hap_loc_end: *const u64,
        hap_is_ref: *const u8,
        max_mnp_distance: u32,
        padding: *const u32,
        region_status: *mut i32,
        variation_present: *mut u8,
        variant_start: *mut u64,
        variant_end: *mut u64,
        padded_start: *mut u64,
        padded_end: *mut u64,
        new_active_start: *mut u64,
        new_active_end: *mut u64,
        new_padded_start: *mut u64,
        new_padded_end: *mut u64,
        hap_fate: *mut i32,
        hap_dup_of: *mut u32,
        out_region_hap_off: *mut u32,
        out_hap_off: *mut u32,
        out_hap_bases: *mut u8,
        out_hap_cigar_off: *mut u32,
        out_hap_cigar: *mut u32,
        out_hap_start_wrt_ref: *mut u32,
        out_hap_source: *mut u32,
        out_hap_is_ref: *mut u8,
        out_region_ref_hap: *mut i32,
    ) -> c_int;
    /// pop_ready_assembly_regions over the band-passed lists of phmm_activity_profile (activity_profile.rs:371-668) and, with
    /// the read arrays, the staged reads each region's fetch returns (assembly_region_iterator.rs:54-159 without BAM I/O);
    /// `capacity` / `required`: regions, membership entries; f32 arrays as `c_void`, the threshold an f64 that holds an f32
    pub fn phmm_assembly_regions(
        h: *mut phmm_handle,
        n_profiles: u32,
        n_windows: u32,
        n_samples: u32,
        assembly_region_extension: u32,
        min_region_size: u32,
        max_region_size: u32,
        max_prob_propagation: u32,
        active_prob_threshold: f64,
        max_input_depth: u32,
        n_prob: u32,
        profile_prob: *const c_void,
        profile_first: *const u32,
        profile_len: *const u32,
        profile_start: *const u64,
        profile_stop: *const u64,
        profile_contig_length: *const u64,
        profile_window: *const u32,
        group_read_off: *const u32,
        read_pos: *const i64,
        read_cigar_off: *const u32,
        read_cigar: *const u32,
        read_off: *const u32,
        read_quals: *const u8,
        capacity: *const u32,
        required: *mut u32,
        profile_status: *mut i32,
        profile_region_off: *mut u32,
        region_start: *mut u64,
        region_end: *mut u64,
        region_padded_start: *mut u64,
        region_padded_end: *mut u64,
        region_states: *mut u32,
        region_flags: *mut u32,
        region_density: *mut c_void,
        region_n_reads: *mut u32,
        region_read_off: *mut u32,
        region_reads: *mut u32,
        read_mean_qual: *mut f64,
    ) -> c_int;

    pub fn phmm_set_switch(h: *mut phmm_handle, name: *const c_char, value: c_int) -> c_int;
    pub fn phmm_get_stat(h: *mut phmm_handle, name: *const c_char) -> u64;
    /// (developer runs: the task records of the device's region server, 72 bytes each)
    pub fn phmm_server_trace(device_id: c_int, out: *mut c_void, cap: u32) -> u32;
    /// "activity=<hash> asm=<hash> cigar=<hash> events=<hash> finalize=<hash> genotype=<hash> pairhmm=<hash> phase=<hash> regions=<hash> server=<hash> sw=<hash> trim=<hash>": the kernel sources the library was built from
    pub fn phmm_build_info() -> *const c_char;

    pub fn phmm_table_eps(eps: *mut *const f64) -> usize;
    pub fn phmm_table_match_to_match(mm: *mut *const f64) -> usize;
    pub fn phmm_table_jacobian(table: *mut *const f64) -> usize;
}
