"""ctypes binding of libphmm.so (the C ABI declared in include/phmm.h).

The library is built in-tree by `__graft_entry__.build()` (or `make -C lorikeet_amd/csrc`).
There is deliberately NO fallback: if the shared library is missing, or no HIP device is
present when an engine is created, this module raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libphmm.so")

u8p = C.POINTER(C.c_uint8)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
f64p = C.POINTER(C.c_double)

PHMM_FLAG_NO_TRISTATE = 1
PHMM_FLAG_F32_FIRST = 2  # opt-in: f32 sweep first, f64 redo of what f32 cannot be trusted with (include/phmm.h)
PHMM_OK = 0
PHMM_ERR_INVALID_ARG = 1
PHMM_ERR_NO_DEVICE = 2
PHMM_ERR_HIP = 3
PHMM_ERR_POSITIVE_RESULT = 4
PHMM_ERR_NOT_BOUND = 5
PHMM_ERR_NO_MEMORY = 6
PHMM_ERR_INTERNAL = 7
PHMM_ERR_CIGAR_CAPACITY = 8
PHMM_ERR_EVENT_CAPACITY = 9
PHMM_SW_SOFTCLIP, PHMM_SW_INDEL, PHMM_SW_LEADING_INDEL, PHMM_SW_IGNORE = 0, 1, 2, 3
PHMM_SW_NO_REFERENCE = 0xffffffff
PHMM_PROJECT_REALIGNED, PHMM_PROJECT_UNCHANGED = 0, 1
PHMM_REGION_SKIP_SINGLE_ALLELE = 1
PHMM_AF_KIND_PLAIN, PHMM_AF_KIND_SPAN_DEL, PHMM_AF_KIND_NON_REF = 0, 1, 2
PHMM_AF_CALLED, PHMM_AF_LOW_QUAL, PHMM_AF_MONOMORPHIC, PHMM_AF_TOO_MANY_ALLELES, PHMM_AF_NOT_CONVERGED = 1, 2, 4, 8, 16
PHMM_AF_ALLELE_PLAUSIBLE, PHMM_AF_ALLELE_OUTPUT = 1, 2
PHMM_GT_USE_PLS, PHMM_GT_USE_POSTERIORS = 0, 1
PHMM_GT_SAMPLE_UNINFORMATIVE, PHMM_GT_SAMPLE_NON_REF_BEST, PHMM_GT_SAMPLE_REF_ONLY = 1, 2, 4
PHMM_ANN_NO_AD, PHMM_ANN_NO_QD, PHMM_ANN_QD_JITTER = 1, 2, 4
PHMM_EVENTS_MAX_REF, PHMM_EVENTS_MAX_HAPS = 16384, 512
PHMM_EV_HAP_IN_TWO_ALLELES = 1
PHMM_EV_TYPE_SNP, PHMM_EV_TYPE_MNP, PHMM_EV_TYPE_INDEL = 1, 2, 3
PHMM_ACTIVITY_MAX_PLOIDY, PHMM_ACTIVITY_MAX_FILTER = 64, 65536
PHMM_ACT_STATUS_REF_SKIP, PHMM_ACT_STATUS_CIGAR_OVERRUN = -1, -2
PHMM_FIN_SOFT_CLIPS, PHMM_FIN_LOW_QUAL_ENDS, PHMM_FIN_ADAPTOR, PHMM_FIN_REGION, PHMM_FIN_PAIRS, PHMM_FIN_ALL = 1, 2, 4, 8, 16, 31
PHMM_FIN_STATUS_CIGAR, PHMM_FIN_STATUS_CLIP_RANGE, PHMM_FIN_STATUS_ARITHMETIC, PHMM_FIN_STATUS_PAIR, PHMM_FIN_STATUS_WORKSPACE = -1, -2, -3, -4, -5
PHMM_PH_NO_TRIM, PHMM_PH_ABORTED, PHMM_PH_GT_01, PHMM_PH_GT_10 = 1, 1, 0, 1
PHMM_ASM_MAX_K_VALUES, PHMM_ASM_MAX_K, PHMM_ASM_MAX_REF_BASES, PHMM_ASM_MAX_READ_BASES, PHMM_ASM_MAX_POSITIONS = 8, 255, 16384, 16384, 536870912
PHMM_ASM_REF_SHORT, PHMM_ASM_REF_NON_UNIQUE, PHMM_ASM_LOW_COMPLEXITY = 1, 2, 4
PHMM_ASM_KMER_NON_UNIQUE, PHMM_ASM_KMER_THREADED, PHMM_ASM_KMER_THREAD_START, PHMM_ASM_KMER_FIRST = 1, 2, 4, 8
PHMM_GRAPH_MAX_SAMPLES, PHMM_GRAPH_MAX_PRUNING_SAMPLES, PHMM_GRAPH_VERTEX_TRACKED, PHMM_GRAPH_VERTEX_REF_SOURCE = 64, 8, 1, 2
PHMM_PRUNE_OP_CHAINS, PHMM_PRUNE_OP_CONNECT, PHMM_PRUNE_HAS_CYCLE, PHMM_PRUNE_NO_REF_ENDS = 1, 2, 1, 2
PHMM_PRUNE_ABSENT, PHMM_PRUNE_REMOVED_CHAINS, PHMM_PRUNE_REMOVED_CONNECT, PHMM_PRUNE_DANGLING_TAIL, PHMM_PRUNE_DANGLING_HEAD = 1, 2, 4, 8, 16
PHMM_RECOVER_OP_TAILS, PHMM_RECOVER_OP_HEADS, PHMM_RECOVER_KIND_TAIL, PHMM_RECOVER_KIND_HEAD = 1, 2, 0, 1
(PHMM_RECOVER_END_NO_PATH, PHMM_RECOVER_END_LOOP, PHMM_RECOVER_END_AT_REF_END, PHMM_RECOVER_END_TOO_SHORT, PHMM_RECOVER_END_CIGAR_NOT_OKAY,
 PHMM_RECOVER_END_TOO_FEW_MATCHING, PHMM_RECOVER_END_WHOLE_INSERTION, PHMM_RECOVER_END_TOO_MANY_MISMATCHES, PHMM_RECOVER_END_CANNOT_PUSH_REF,
 PHMM_RECOVER_END_CANNOT_EXTEND, PHMM_RECOVER_END_MERGED, PHMM_RECOVER_END_NO_MERGE_POINT, PHMM_RECOVER_END_REFERENCE_FAILS) = range(13)
PHMM_SEQ_OK, PHMM_SEQ_SKIPPED, PHMM_SEQ_REFERENCE_FAILS = 0, 1, 2
(PHMM_PATHS_OK, PHMM_PATHS_SKIPPED, PHMM_PATHS_NO_ENDS, PHMM_PATHS_NO_PATH, PHMM_PATHS_CYCLES_STAY, PHMM_PATHS_WEIGHT_RANGE,
 PHMM_PATHS_BUDGET) = range(7)
PHMM_PATHS_MAX_WEIGHT, PHMM_PATHS_EQUALS_REF = 1 << 20, 0xfffffffe
PHMM_REG_ACTIVE, PHMM_REG_FORCED, PHMM_REG_OVER_DEPTH = 1, 2, 4
PHMM_REG_STATUS_MIN_REGION_SIZE, PHMM_REG_STATUS_START_PAST_CONTIG = -1, -2
PHMM_EV_STATUS_BAD_OPERATOR, PHMM_EV_STATUS_BLOCK, PHMM_EV_STATUS_MERGE, PHMM_EV_STATUS_CIGAR_OVERRUN, PHMM_EV_STATUS_ALLELES = -1, -2, -3, -4, -5

class EngineConfig(C.Structure):
    """phmm_engine_config (include/phmm.h)."""
    _fields_ = [("constant_gcp", C.c_uint8), ("pcr_error_model", C.c_uint8),
                ("base_quality_score_threshold", C.c_uint8), ("dynamic_read_disqualification", C.c_uint8),
                ("symmetrically_normalize_alleles_to_reference", C.c_uint8),
                ("disable_cap_read_qualities_to_mapq", C.c_uint8), ("reserved", C.c_uint8 * 2),
                ("log10_global_read_mismapping_rate", C.c_double), ("read_disqualification_scale", C.c_double),
                ("expected_error_rate_per_base", C.c_double)]


class SwParameters(C.Structure):
    """phmm_sw_parameters == gkl::smithwaterman::Parameters::new(match, mismatch, gap open, gap extend)."""
    _fields_ = [("match_value", C.c_int32), ("mismatch_penalty", C.c_int32), ("gap_open_penalty", C.c_int32),
                ("gap_extend_penalty", C.c_int32)]


class RealignConfig(C.Structure):
    """phmm_realign_config (include/phmm.h)."""
    _fields_ = [("sw_parameters", SwParameters), ("overhang_strategy", C.c_int32), ("flags", C.c_uint32),
                ("informative_threshold", C.c_double)]


class RecoverConfig(C.Structure):
    """phmm_recover_config (include/phmm.h)."""
    _fields_ = [("ops", C.c_uint32), ("min_dangling_branch_length", C.c_int32), ("min_matching_bases", C.c_int32),
                ("max_mismatches_in_dangling_head", C.c_int32), ("num_pruning_samples", C.c_uint32), ("sw_parameters", SwParameters)]


class FinalizeConfig(C.Structure):
    """phmm_finalize_config (include/phmm.h)."""
    _fields_ = [("steps", C.c_uint32), ("min_tail_quality", C.c_uint8), ("dont_use_soft_clipped_bases", C.c_uint8),
                ("half_of_pcr_snv_qual", C.c_uint8), ("reserved", C.c_uint8)]


class PlanInfo(C.Structure):
    """phmm_plan_info (include/phmm.h)."""
    _fields_ = [("cells", C.c_uint64), ("chain_cells", C.c_uint64), ("chain_items", C.c_uint64), ("n_launches", C.c_uint32),
                ("n_chain_launches", C.c_uint32), ("min_reads_per_run", C.c_uint32), ("reserved", C.c_uint32),
                ("dominant_kernel", C.c_char * 64), ("swept_cells", C.c_uint64), ("pad_column_cells", C.c_uint64),
                ("pad_slot_cells", C.c_uint64)]


_REGION_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, u32p, u32p, u32p, u8p, u8p, u8p, u8p, u8p, u32p, u32p, u8p,
                C.POINTER(C.c_int32), u64p, C.POINTER(C.c_int32), u64p, u32p, u32p, u32p, u32p, u32p, u64p, f64p, u8p,
                C.POINTER(C.c_int32), f64p, f64p, u32p, u32p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]

# every symbol include/phmm.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("phmm_device_count", C.c_int, []),
    ("phmm_create", C.c_void_p, [C.c_int, C.c_uint]),
    ("phmm_destroy", None, [C.c_void_p]),
    ("phmm_last_error", C.c_char_p, [C.c_void_p]),
    ("phmm_compute", C.c_int, [C.c_void_p, C.c_uint32, u32p, u32p, u32p, u8p, u8p, u8p, u8p, u8p, u32p, u8p, u64p, f64p]),
    ("phmm_submit", C.c_int, [C.c_void_p, C.c_uint32, u32p, u32p, u32p, u8p, u8p, u8p, u8p, u8p, u32p, u8p, u64p, f64p,
                              C.POINTER(C.c_uint64)]),
    ("phmm_wait", C.c_int, [C.c_void_p, C.c_uint64]),
    ("phmm_submit_stats", None, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("phmm_assign_regions", C.c_int, [C.c_uint32, u32p, u32p, u32p, u32p, C.c_uint32, u32p]),
    ("phmm_split_regions", C.c_int, [C.c_uint32, u32p, u32p, u32p, u32p, C.c_uint32, u32p]),
    ("phmm_compute_multi", C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, u32p, u32p, u32p, u8p, u8p, u8p, u8p, u8p,
                                     u32p, u8p, u64p, f64p]),
    ("phmm_batch_create", C.c_void_p, [C.c_void_p, C.c_uint32, u32p, u32p, u32p, u32p, u64p]),
    ("phmm_batch_destroy", None, [C.c_void_p]),
    ("phmm_batch_bind_device", C.c_int, [C.c_void_p] + [C.c_void_p] * 7),
    ("phmm_batch_upload", C.c_int, [C.c_void_p, u8p, u8p, u8p, u8p, u8p, u8p]),
    ("phmm_batch_launch", C.c_int, [C.c_void_p, C.c_void_p]),
    ("phmm_batch_download", C.c_int, [C.c_void_p, f64p]),
    ("phmm_batch_status", C.c_int, [C.c_void_p]),
    ("phmm_batch_cells", C.c_uint64, [C.c_void_p]),
    ("phmm_batch_algorithmic_bytes", C.c_uint64, [C.c_void_p]),
    ("phmm_batch_num_launches", C.c_uint32, [C.c_void_p]),
    ("phmm_batch_executed_cells", C.c_uint64, [C.c_void_p]),
    ("phmm_batch_dominant_kernel", C.c_char_p, [C.c_void_p]),
    ("phmm_plan_describe", C.c_int, [C.c_uint, C.c_uint32, C.c_uint32, u32p, u32p, u32p, u32p, C.POINTER(PlanInfo)]),
    ("phmm_engine_compute", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, u32p, u32p, u32p, u8p, u8p, u8p, u8p, u8p,
                                      u32p, u8p, C.POINTER(C.c_int32), u64p, f64p, u8p]),
    ("phmm_engine_submit", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, u32p, u32p, u32p, u8p, u8p, u8p, u8p, u8p,
                                     u32p, u8p, C.POINTER(C.c_int32), u64p, f64p, u8p, C.POINTER(C.c_uint64)]),
    ("phmm_engine_compute_multi", C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_uint32, u32p, u32p, u32p, u8p, u8p, u8p, u8p, u8p,
                                            u32p, u8p, C.POINTER(C.c_int32), u64p, f64p, u8p]),
    ("phmm_sw_align", C.c_int, [C.c_void_p, C.c_uint32, u32p, u8p, u32p, u8p, C.c_void_p, C.c_int, u64p, u32p, u32p,
                                C.POINTER(C.c_int32)]),
    ("phmm_sw_align_indexed", C.c_int, [C.c_void_p, C.c_uint32, u32p, u8p, C.c_uint32, u32p, u32p, u8p, C.c_void_p, C.c_int, u64p,
                                        u32p, u32p, C.POINTER(C.c_int32)]),
    ("phmm_best_alleles", C.c_int, [C.c_void_p, C.c_uint32, u32p, u32p, u64p, f64p, u8p, C.POINTER(C.c_int32), C.c_double,
                                    C.POINTER(C.c_int32), f64p, f64p]),
    ("phmm_realign_to_best", C.c_int, [C.c_void_p, C.c_uint32, u32p, u32p, u32p, u8p, u32p, u8p, u64p, f64p, u8p,
                                       C.POINTER(C.c_int32), C.c_double, C.c_void_p, C.c_int, u64p, u32p, u32p,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32), f64p, f64p]),
    ("phmm_project_to_reference", C.c_int, [C.c_void_p, C.c_uint32, u32p, u32p, u32p, u8p, u32p, u8p, C.POINTER(C.c_int32), u64p, u32p, u32p,
                                            u32p, C.POINTER(C.c_int32), u64p, u32p, u32p, C.POINTER(C.c_int32), u32p, u32p, u64p, u32p, u32p,
                                            C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    ("phmm_realign_reads", C.c_int, [C.c_void_p, C.c_uint32, u32p, u32p, u32p, u8p, u32p, u8p, u64p, f64p, u8p, C.POINTER(C.c_int32), C.c_double,
                                     C.c_void_p, C.c_int, C.POINTER(C.c_int32), u64p, u32p, u32p, u32p, u32p, u32p, u64p, u32p, u32p,
                                     C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), f64p, f64p]),
    ("phmm_region_compute", C.c_int, _REGION_ARGS),
    ("phmm_region_submit", C.c_int, _REGION_ARGS + [C.POINTER(C.c_uint64)]),
    ("phmm_region_compute_multi", C.c_int, [C.POINTER(C.c_void_p), C.c_uint32] + _REGION_ARGS[1:]),
    ("phmm_calculate_cigar", C.c_int, [C.c_void_p, C.c_uint32, u32p, u8p, u32p, u8p, C.c_void_p, C.c_int, u64p, u32p, u32p, C.POINTER(C.c_int32)]),
    ("phmm_genotype_count", C.c_uint32, [C.c_uint32, C.c_uint32]),
    ("phmm_genotype_likelihoods", C.c_int, [C.c_void_p, C.c_uint32, u32p, u32p, u64p, f64p, u8p, u32p, C.POINTER(C.c_int64),
                                            C.POINTER(C.c_int64), C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p, C.POINTER(C.c_int64),
                                            C.POINTER(C.c_int64), C.POINTER(C.c_int32), u64p, f64p, C.POINTER(C.c_int32), u32p]),
    ("phmm_allele_frequency", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p, u8p, u64p, C.POINTER(C.c_int32),
                                        C.c_double, C.c_double, C.c_double, C.c_double, f64p, f64p, f64p, C.POINTER(C.c_int64), u8p,
                                        f64p, u32p, u32p]),
    ("phmm_assign_genotypes", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p, u8p, u64p, C.POINTER(C.c_int32),
                                        u32p, u32p, C.c_uint32, C.c_double, C.c_double, u8p, u64p, C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32), f64p, u8p, u8p, f64p, f64p, f64p]),
    ("phmm_annotate_events", C.c_int, [C.c_void_p, C.c_uint32, u32p, u32p, u64p, f64p, u8p, u32p, C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int64), u8p, C.c_uint32, C.c_uint32, u32p, u32p, C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int32), u32p, u32p, u32p, u8p, u64p, u32p, u32p,
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64), u8p, f64p, u32p, C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32), f64p, u32p, u8p, u8p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       f64p, u32p]),
    ("phmm_discover_events", C.c_int, [C.c_void_p, C.c_uint32, u32p, u8p, u64p, u64p, u64p, u64p, u32p, u32p, u8p, u32p, u32p, u32p,
                                       C.c_uint32, C.c_int, C.c_uint32, u32p, u32p, u32p, C.POINTER(C.c_int32), u32p, u32p,
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int64), u32p, C.POINTER(C.c_int32), u32p, u8p, u32p, u8p, u32p,
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64), u32p, u32p, u8p, u32p]),
    ("phmm_activity_profile", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double,
                                        C.c_double, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_uint32, u64p, u32p, u64p, u32p, u8p,
                                        u32p, C.POINTER(C.c_int64), u32p, u32p, u32p, u8p, u8p, C.POINTER(C.c_int32), u32p, u32p, u32p,
                                        f64p, C.POINTER(C.c_int32), f64p, u32p, f64p, u32p, C.c_void_p, u32p, C.c_void_p, u32p]),
    ("phmm_activity_band_kernel", C.c_int, [C.c_uint32, C.c_double, C.c_int, u32p, f64p]),
    ("phmm_activity_term_table", C.c_int, [C.c_uint32, f64p]),
    ("phmm_finalize_reads", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, u32p, u64p, u64p, C.POINTER(C.c_int64),
                                      C.c_void_p, u8p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), u32p, u32p, u32p, u8p, u8p,
                                      C.POINTER(C.c_int32), u64p, C.POINTER(C.c_int32), u8p, C.POINTER(C.c_int64), u8p, u32p, u32p, u32p,
                                      u32p, u32p, u32p, u32p, u8p]),
    ("phmm_phase_calls", C.c_int, [C.c_void_p, C.c_uint32, u32p, u32p, u32p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), u32p, u8p, u32p,
                                   u8p, u32p, C.POINTER(C.c_int64), u32p, u8p, u32p, u32p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int32),
                                   C.c_uint32, u32p, C.POINTER(C.c_int64), u32p, u8p, C.POINTER(C.c_int32), u8p, C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int64), u32p, u32p, u8p, C.POINTER(C.c_int32)]),
    ("phmm_assembly_kmers", C.c_int, [C.c_void_p, C.c_uint32, u32p, u8p, u32p, u32p, u8p, u8p, u32p, u32p, C.c_uint32, u32p, C.c_uint32,
                                      u32p, u32p, u32p, u32p, u32p, u8p, u8p, u32p, u32p]),
    ("phmm_assembly_graph", C.c_int, [C.c_void_p, C.c_uint32, u32p, u8p, u32p, u32p, u8p, u8p, u32p, u32p, u32p, C.c_uint32, u32p, C.c_uint32,
                                      C.c_uint32, u32p, u32p, u32p, u32p, u32p, u32p, u32p, u32p, u32p, u32p, u32p, u8p, u32p, u32p, u8p,
                                      u32p, u32p, u32p, u32p, u32p]),
    ("phmm_assembly_prune", C.c_int, [C.c_void_p, C.c_uint32, u32p, u32p, u32p, u32p, u8p, u32p, u8p, u8p, C.c_uint32, u32p, u32p, u32p, u32p,
                                      u32p, u32p, u32p, u32p, u32p, u8p, u8p]),
    ("phmm_assembly_recover", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, u32p, u8p, u32p, u32p, u8p, u32p, u32p, C.c_uint32, u32p, u32p, u32p, u32p,
                                        u32p, u32p, u32p, u8p, u32p, u32p, u8p, u8p, u32p, u32p, u32p, u32p] + [u32p] * 22 + [u8p, u8p]),
    ("phmm_assembly_seqgraph", C.c_int, [C.c_void_p, C.c_uint32, u32p, u8p, u32p, u32p, u8p, u32p, u32p, C.c_uint32, u32p, u32p, u32p, u32p, u32p,
                                         u32p, u32p, u8p, u32p, u32p, u8p, u8p, u8p, u32p, u32p, u32p] + [u32p] * 17 + [u8p, u32p, u8p, u32p]),
    ("phmm_assembly_best_paths", C.c_int, [C.c_void_p, C.c_uint32, u32p, u32p, u32p, u32p, u32p, u32p, u8p, u32p, u8p, u32p, u32p, u32p, u8p,
                                            C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u32p, u8p, u32p, u32p] + [u32p] * 8 +
                                           [f64p, u8p, u32p, u32p, u32p, u32p, u8p, u8p, u8p]),
    ("phmm_trim_regions", C.c_int, [C.c_void_p, C.c_uint32, u32p, u8p, u64p, u64p, u64p, u64p, u64p, u32p, u32p, u8p, u32p, u32p, u32p,
                                    u64p, u64p, u8p, C.c_uint32, u32p, C.POINTER(C.c_int32), u8p, u64p, u64p, u64p, u64p, u64p, u64p,
                                    u64p, u64p, C.POINTER(C.c_int32), u32p, u32p, u32p, u8p, u32p, u32p, u32p, u32p, u8p,
                                    C.POINTER(C.c_int32)]),
    ("phmm_assembly_regions", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.c_double, C.c_uint32, C.c_uint32, C.c_void_p, u32p, u32p, u64p, u64p, u64p, u32p, u32p,
                                        C.POINTER(C.c_int64), u32p, u32p, u32p, u8p, u32p, u32p, C.POINTER(C.c_int32), u32p, u64p, u64p,
                                        u64p, u64p, u32p, u32p, C.c_void_p, u32p, u32p, u32p, f64p]),
    ("phmm_set_switch", C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    ("phmm_get_stat", C.c_uint64, [C.c_void_p, C.c_char_p]),
    ("phmm_build_info", C.c_char_p, []),
    ("phmm_server_trace", C.c_uint32, [C.c_int, C.c_void_p, C.c_uint32]),
    ("phmm_table_eps", C.c_size_t, [C.POINTER(f64p)]),
    ("phmm_table_match_to_match", C.c_size_t, [C.POINTER(f64p)]),
    ("phmm_table_jacobian", C.c_size_t, [C.POINTER(f64p)]),
]

_lib = None


def load():
    """Load libphmm.so and bind every symbol of include/phmm.h.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "lorikeet_amd: %s not found -- the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)." % LIB_PATH)
    # One HIP runtime per process: PyTorch ships its own libamdhip64; if libphmm.so pulled in the system
    # copy first, torch's later initialisation would see "No HIP GPUs".  Import torch first (when it is
    # installed) so both resolve to the same runtime.  Plain C / Rust callers link the system runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
