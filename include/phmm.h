/*
 * phmm.h -- C ABI of the MI355X-native PairHMM read x haplotype likelihood engine.
 *
 * This is the drop-in boundary for Lorikeet's PairHMM path.  The reference has no FFI of its
 * own on this path; the seam it does have is the function pointer returned by
 * `gkl::pairhmm::forward()` and the batch loop around it:
 *
 *   reference/src/pair_hmm/pair_hmm.rs:345-375   PairHMM::compute_likelihoods
 *       for read { for hap { forward(hap, read, read_quals, ins_gop, del_gop, gcp) -> f64 } }
 *       => m_log_likelihood_array, Nr*Nh f64, READ-MAJOR, haplotypes in initialize() order
 *   reference/src/pair_hmm/pair_hmm.rs:217-341   PairHMM::compute_log10_likelihoods (caller)
 *   reference/tests/vector_pair_hmm_unit_tests.rs:51-59   the same call shape in the tests
 *
 * Every entry point below takes plain pointers and sizes (no C++/torch types).  Inputs are the
 * arrays the Rust call site already holds (`ReadDataHolder`, pair_hmm.rs:720-745, and
 * `m_haplotype_data_array`, :71-79) flattened into struct-of-arrays with prefix-sum offsets, so
 * that any number of assembly regions travel in one call.  INTEGRATION.md shows the Rust
 * `extern "C"` block and the `AVXMode::Hip` arm that binds them.
 *
 * Semantics (identical to the reference):
 *   - log10 Pr(read | haplotype) of the M/I/D forward recurrence of pair_hmm.rs:503-615,
 *     tristate correction ON unless PHMM_FLAG_NO_TRISTATE (pair_hmm.rs:189-191, :643-651);
 *   - base comparison is raw byte equality, uppercase 'N' on either side is a wildcard (:643);
 *   - qualities are full u8 (0..=255); reads longer than the haplotype are legal; an empty read
 *     gives -inf; an empty read list is a no-op (:224); an EMPTY HAPLOTYPE is rejected with
 *     PHMM_ERR_INVALID_ARG by every entry point (the reference would divide 2^1020 by zero and return
 *     -inf for every read of the region, :515-517; Lorikeet's assembler never produces one);
 *   - every result satisfies <= 0.0; a violation (the reference asserts, :478-481) is reported
 *     as PHMM_ERR_POSITIVE_RESULT.
 * Results agree with the reference's scalar f64 path to ~1e-13 absolute in log10 (FMA contraction,
 * exact rescalings of the DP state and the order of the final row sum are the only differences,
 * NOTEBOOK.md §4); the reference's own gate is 1e-5 abs.  Pairs whose log10 likelihood is below -600 --
 * where the reference's 2^1020-scaled sums approach the denormal range and every rounding shows -- are recomputed
 * in the reference's own operation order, so the underflow band (down to and including the point where the result
 * turns to -inf, ~1e-628) agrees with the scalar arm as well.
 *
 * Every entry point returns with the calling thread's current HIP device restored, and no C++ exception crosses
 * the boundary (PHMM_ERR_NO_MEMORY / PHMM_ERR_INTERNAL).  Slots of `out` that out_off leaves between regions
 * (gaps) are never written.
 *
 * Threading: a handle may be used by one thread at a time; create one per host thread (the
 * reference clones its engine per rayon task, assembly_region_walker.rs:227) or serialise.  The exception is
 * phmm_submit / phmm_engine_submit / phmm_wait: any number of threads may call them on ONE shared handle, and the
 * library computes the regions of all waiting threads together.  phmm_compute_multi spreads one call over several
 * handles (one per device).
 * There is NO CPU fallback: without a HIP device phmm_create() fails.
 */
#ifndef PHMM_H
#define PHMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHMM_VERSION 1

/* flags for phmm_create */
#define PHMM_FLAG_NO_TRISTATE 1u /* PairHMM::do_not_use_tristate_correction (pair_hmm.rs:189) */
#define PHMM_FLAG_F32_FIRST 2u   /* opt-in: what the reference's vector arm does (gkl, called at pair_hmm.rs:345-375):
                                  * large batches are swept in f32 first and every read whose result is too small to
                                  * trust in f32 (< ~1e-59 / haplotype length), or that needs the general path, is
                                  * recomputed in f64.  Results of the f32 pairs differ from the f64 path by f32
                                  * rounding (<= 2e-6 in log10 measured, the reference's gate is 1e-5); default OFF:
                                  * everything in f64.  Small calls, and region calls that go through the resident region
                                  * server, are computed in f64 under this flag too (NOTEBOOK.md 20.7). */

/* status codes (0 == success) */
#define PHMM_OK 0
#define PHMM_ERR_INVALID_ARG 1      /* null pointer, non-monotonic offsets, size mismatch      */
#define PHMM_ERR_NO_DEVICE 2        /* no HIP device / bad device id                           */
#define PHMM_ERR_HIP 3              /* a HIP runtime call failed; see phmm_last_error          */
#define PHMM_ERR_POSITIVE_RESULT 4  /* some log10 likelihood > 0 (reference asserts, :478-481) */
#define PHMM_ERR_NOT_BOUND 5        /* phmm_batch_launch before device buffers were bound      */
#define PHMM_ERR_NO_MEMORY 6        /* a host allocation failed (std::bad_alloc never crosses the ABI)    */
#define PHMM_ERR_INTERNAL 7         /* any other C++ exception inside the library; see phmm_last_error    */
#define PHMM_ERR_CIGAR_CAPACITY 8   /* phmm_sw_align: a CIGAR did not fit its slot; n_cigar has the sizes */
#define PHMM_ERR_EVENT_CAPACITY 9   /* phmm_discover_events: an output array is too small; required has the sizes */

typedef struct phmm_handle phmm_handle;
typedef struct phmm_batch phmm_batch;

/* Number of HIP devices visible to the process (0 if none / no driver). */
int phmm_device_count(void);

/* Create an engine on HIP device `device_id`.  Builds the quality->probability tables
 * (quality_utils.rs:82-104, pair_hmm_model.rs:47-78) once and keeps them resident in HBM;
 * owns a stream, pinned staging and device arenas that grow on demand.  While at most four engines are alive on a device,
 * each runs its one-enqueue calls on a hardware queue of its own (callers with an engine each then run side by side whatever
 * the runtime does with ordinary streams); env PHMM_REGION_OWN_QUEUE=0 at creation turns that off.
 * While MORE than five of the caller's engines are alive on a device (an engine per worker thread at Lorikeet's --threads 10),
 * the one-shot phmm_region_compute calls of such a private engine are served by the device's resident REGION SERVER (a kernel
 * that stays on the chip while calls keep coming: the region is staged into a slot of pinned memory, every read runs as one wave
 * from pre-step to projection, nothing is launched; phmm_server.cpp).  Results and error reporting are the call's own, and the
 * likelihoods are the region's own bits whatever else is in flight (16 lanes x ceil(H / 16) columns per pair: a function of the
 * region's longest haplotype).  Calls outside the server's limits (reads beyond 268 bases, haplotypes beyond 512, more than 1 MB of
 * inputs) take the engine's own streams.  env PHMM_REGION_SERVER=0 turns the server off, =1 sends every region call through it.
 * While the caller holds more engines on a device than the process has cores (its affinity mask, its container's CPU quota), a
 * one-shot call waits for its kernels in 20 us naps instead of spinning: spinning waiters beyond the cores are throttled together
 * with the callers that stage (32 engines on 16 cores ran at half the rate of 16; NOTEBOOK.md 20.5).
 * Opt-in, env PHMM_ROUTE_SHARED=n: while more than n engines are alive, the one-shot calls of private engines -- phmm_compute,
 * phmm_engine_compute, phmm_region_compute on up to eight regions or 512 KB per array -- go through ONE shared engine of the same
 * flags inside the library instead (the queue of phmm_submit: callers that are waiting anyway share a flush); which regions share a
 * launch depends on timing, so likelihoods are then reproducible to ~1e-13 rather than bit for bit.  An engine whose developer
 * switches were set (phmm_set_switch) keeps to its own streams.
 * Debug environment: PHMM_MIRROR_CANARY=1 makes a device store that lands in the pinned hand-over buffer outside its call fail
 * that call (PHMM_ERR_INTERNAL; =2: abort); PHMM_REGION_PICK_TIMEOUT_US (default 5 000) bounds the small region call's wait for
 * its second hardware queue -- out of time, the call is redone the chained way (phmm_get_stat "region_pick_timeouts").
 * Replaces PairHMM::initialize's per-region table/matrix construction (pair_hmm.rs:63-165).
 * Returns NULL on failure (phmm_last_error(NULL) has the message). */
phmm_handle *phmm_create(int device_id, unsigned flags);
void phmm_destroy(phmm_handle *h);

/* Last error message of this handle (or of the failed phmm_create when h == NULL).
 * Never NULL; valid until the next call on the same handle. */
const char *phmm_last_error(phmm_handle *h);

/*
 * Synchronous whole-batch call on HOST buffers (pageable is fine): plan, H2D, kernels, D2H.
 * Replaces PairHMM::compute_likelihoods (pair_hmm.rs:345-375) for `n_regions` regions at once.
 *
 *   region_read_off[n_regions+1]  prefix sums: region g owns reads  [region_read_off[g], region_read_off[g+1])
 *   region_hap_off [n_regions+1]  prefix sums: region g owns haps   [region_hap_off[g],  region_hap_off[g+1])
 *   read_off[n_reads+1]           byte offsets of each read into the five per-base read arrays
 *   read_bases, base_q, ins_q, del_q, gcp   read_off[n_reads] bytes each (ReadDataHolder fields)
 *   hap_off[n_haps+1], hap_bases  byte offsets / bases of each haplotype
 *   out_off[n_regions+1]          element offsets into out; region g needs Nr_g*Nh_g doubles
 *   out                           per region row-major [read][hap] == m_log_likelihood_array order
 *
 * All pointers are caller-owned and not retained.  Returns a PHMM_* status.
 */
int phmm_compute(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off,
                 const uint32_t *region_hap_off, const uint32_t *read_off, const uint8_t *read_bases,
                 const uint8_t *base_q, const uint8_t *ins_q, const uint8_t *del_q, const uint8_t *gcp,
                 const uint32_t *hap_off, const uint8_t *hap_bases, const uint64_t *out_off, double *out);

/*
 * Cross-thread batching: the same call as phmm_compute, split into submit + wait, and -- unlike every other entry
 * point -- safe to call from many threads on ONE shared handle.  This is the call pattern of the reference as it
 * stands: every rayon worker calls PairHMM::compute_likelihoods (pair_hmm.rs:345-375) with one region at a time
 * (assembly_region_walker.rs:210-273).  A submission is only queued.  The first thread to wait while an engine lane is
 * free leads one flush: it takes everything queued so far (its own region plus those of the workers that arrived in
 * the meantime), computes it as one batch and hands every region's results to its owner; the other threads sleep until
 * theirs are in.  No timer, no background thread: batches become as large as the number of workers that were waiting
 * anyway, a lone caller pays nothing.  Results are those of phmm_compute on the same regions (every region is
 * independent; which regions share a launch only selects the kernel shape, like batch size does in phmm_compute).
 *
 *   phmm_submit   same arrays as phmm_compute; ALL of them, inputs and `out`, stay caller-owned and must remain valid
 *                 until phmm_wait(ticket) has returned.  Argument errors are reported here (nothing is queued).
 *   phmm_wait     blocks until the ticket's results are in `out`; returns that submission's own status (a failure in
 *                 another thread's region does not leak into it).  Each ticket must be waited for exactly once.
 * phmm_last_error() after a failed phmm_submit / phmm_wait returns the calling thread's message.
 */
int phmm_submit(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off,
                const uint32_t *region_hap_off, const uint32_t *read_off, const uint8_t *read_bases,
                const uint8_t *base_q, const uint8_t *ins_q, const uint8_t *del_q, const uint8_t *gcp,
                const uint32_t *hap_off, const uint8_t *hap_bases, const uint64_t *out_off, double *out,
                uint64_t *ticket);
int phmm_wait(phmm_handle *h, uint64_t ticket);
/* How many flushes have run on this handle and how many submissions they carried (batching achieved). */
void phmm_submit_stats(phmm_handle *h, uint64_t *n_flushes, uint64_t *n_submissions);

/*
 * Several devices, one process (regions shard, nothing is exchanged).  phmm_compute_multi is phmm_compute over
 * `n_handles` engines, normally one per device.  Whole regions go to engines in CONTIGUOUS ranges balanced by
 * cells(region) = sum of read lengths x sum of haplotype lengths (phmm_split_regions); only when such ranges come out
 * more than 5 % uneven -- a heavy-tailed set -- are regions dealt out one by one by greedy longest-processing-time
 * (phmm_assign_regions: heaviest region first onto the least loaded engine).  Either way every engine stages its share
 * straight from the caller's arrays (no gather: each payload byte is copied once, into that engine's pinned staging),
 * computes it concurrently on a host thread of its own pinned to the CPUs local to its GPU, and the results land in the
 * caller's `out` exactly where phmm_compute would put them.  The handles must not be in use by other threads during the
 * call; on failure the message is phmm_last_error(handles[0]).  phmm_assign_regions / phmm_split_regions expose the two
 * assignments alone (host only, no device needed): part_of_region[g] in [0, n_parts); first_region[0..n_parts], part k
 * owning the regions [first_region[k], first_region[k+1]).
 */
int phmm_assign_regions(uint32_t n_regions, const uint32_t *region_read_off, const uint32_t *region_hap_off,
                        const uint32_t *read_off, const uint32_t *hap_off, uint32_t n_parts,
                        uint32_t *part_of_region);
int phmm_split_regions(uint32_t n_regions, const uint32_t *region_read_off, const uint32_t *region_hap_off,
                       const uint32_t *read_off, const uint32_t *hap_off, uint32_t n_parts,
                       uint32_t *first_region);
int phmm_compute_multi(phmm_handle *const *handles, uint32_t n_handles, uint32_t n_regions,
                       const uint32_t *region_read_off, const uint32_t *region_hap_off, const uint32_t *read_off,
                       const uint8_t *read_bases, const uint8_t *base_q, const uint8_t *ins_q, const uint8_t *del_q,
                       const uint8_t *gcp, const uint32_t *hap_off, const uint8_t *hap_bases,
                       const uint64_t *out_off, double *out);

/*
 * Split-phase interface for device-resident data and for overlapping transfers with compute.
 * A batch owns the launch plan (regions binned into kernel shape classes) and the device copy
 * of the offset arrays; the byte payload and the output live in device memory that is either
 * caller-owned (phmm_batch_bind_device) or uploaded from host buffers (phmm_batch_upload).
 *
 *   b = phmm_batch_create(h, <offset arrays on the host>);
 *   phmm_batch_bind_device(b, d_read_bases, ..., d_out);   // or phmm_batch_upload(b, host ptrs)
 *   phmm_batch_launch(b, stream);                           // async: kernels only
 *   ... hipStreamSynchronize / phmm_batch_download(b, out) ...
 *   phmm_batch_destroy(b);
 */
phmm_batch *phmm_batch_create(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off,
                              const uint32_t *region_hap_off, const uint32_t *read_off,
                              const uint32_t *hap_off, const uint64_t *out_off);
void phmm_batch_destroy(phmm_batch *b);

/* Device pointers (on the handle's device), caller-owned, must stay valid until the launch completes. */
int phmm_batch_bind_device(phmm_batch *b, const uint8_t *d_read_bases, const uint8_t *d_base_q,
                           const uint8_t *d_ins_q, const uint8_t *d_del_q, const uint8_t *d_gcp,
                           const uint8_t *d_hap_bases, double *d_out);

/* Copy host payload into batch-owned device buffers (async on the handle's stream) and bind them. */
int phmm_batch_upload(phmm_batch *b, const uint8_t *read_bases, const uint8_t *base_q, const uint8_t *ins_q,
                      const uint8_t *del_q, const uint8_t *gcp, const uint8_t *hap_bases);

/* Enqueue the forward kernels on `stream` (a hipStream_t; NULL = the handle's own stream).
 * Asynchronous; no host<->device copies, no allocation. */
int phmm_batch_launch(phmm_batch *b, void *stream);

/* Wait for the handle's stream, copy batch-owned output to `out` (host) and check the device
 * status word.  Only valid after phmm_batch_upload + phmm_batch_launch(b, NULL). */
int phmm_batch_download(phmm_batch *b, double *out);

/* Read and clear the device status word after the caller synchronised its own stream
 * (for the bind_device flow).  Returns PHMM_OK or PHMM_ERR_POSITIVE_RESULT. */
int phmm_batch_status(phmm_batch *b);

/* Introspection for tests / bench: totals of the plan. */
uint64_t phmm_batch_cells(const phmm_batch *b);           /* sum over regions of (sum R)*(sum H)      */
uint64_t phmm_batch_algorithmic_bytes(const phmm_batch *b); /* sum 5R + sum H + 8*Nr*Nh    */
uint32_t phmm_batch_num_launches(const phmm_batch *b);    /* kernel launches one phmm_batch_launch does */
/* What the planned launches sweep, in lane-cells: every row of every wave x 64 lanes x its columns per lane -- the columns beyond a
 * haplotype's end, the haplotype slots a wave leaves empty.  executed / phmm_batch_cells is what a batch's shapes cost in padding
 * (1.01 for the uniform 150 / 300 batch).  (The reference's scalar arm skips the columns a haplotype shares with the one before it,
 * find_first_position_where_haplotypes_differ, pair_hmm.rs:452-464, 706-717; here every pair is swept in full: a device form of the
 * sharing was built in round 4, measured at x 0.96-1.10 and removed in round 6, NOTEBOOK.md 18.4.) */
uint64_t phmm_batch_executed_cells(const phmm_batch *b);
/* Name of the kernel doing most cells of this batch as rocprofv3 reports it, e.g. "phmm_forward_chain_k<16,19>". */
const char *phmm_batch_dominant_kernel(const phmm_batch *b);

/*
 * The launch plan of a batch WITHOUT a device (host only, like phmm_split_regions): what phmm_batch_create would decide
 * for these offsets on an engine created with `flags`, `concurrent_callers` flows sharing the chip (1 = alone).  For sizing
 * shards before any GPU is touched: e.g. that each rank's share of a set still takes the chained kernel with enough work
 * items (one wave each) to put two waves on every one of the chip's 1 024 SIMDs.
 */
typedef struct phmm_plan_info {
    uint64_t cells;              /* sum over regions of (sum R) x (sum H)                                   */
    uint64_t chain_cells;        /* ... of which the chained kernels sweep                                  */
    uint64_t chain_items;        /* their work items: one wave each (a run of reads x one load of haplotypes) */
    uint32_t n_launches;         /* kernel launches of one phmm_batch_launch                                */
    uint32_t n_chain_launches;
    uint32_t min_reads_per_run;  /* shortest run of reads a chained work item holds (0: nothing chains)     */
    uint32_t reserved;
    char dominant_kernel[64];
    /* What the launches sweep (phmm_batch_executed_cells), in lane-cells = steps x 64 lanes x K columns of every wave ...          */
    uint64_t swept_cells;
    uint64_t pad_column_cells;   /* ... of which columns beyond a haplotype's end (lanes x K - H per pair)                      */
    uint64_t pad_slot_cells;     /* ... haplotype slots a wave leaves empty; the rest above `cells` is steps without a read row */
                                 /*     (SUM / RESET rows between the reads of a run, the fill of the lane pipeline)            */
} phmm_plan_info;
int phmm_plan_describe(unsigned flags, uint32_t concurrent_callers, uint32_t n_regions, const uint32_t *region_read_off,
                       const uint32_t *region_hap_off, const uint32_t *read_off, const uint32_t *hap_off, phmm_plan_info *info);

/*
 * Engine-level call: everything PairHMMLikelihoodCalculationEngine::compute_read_likelihoods does with
 * the numbers (reference src/pair_hmm/pair_hmm_likelihood_calculation_engine.rs:195-242), for
 * n_regions regions at once, on the device:
 *   1. modify_read_qualities (:352-388, default branch): PCR indel error model (:502-611) and the
 *      quality caps (:428-466) on copies of the read qualities; gcp = constant (:649-651);
 *   2. the PairHMM forward kernels on the modified qualities (pair_hmm.rs:345-375);
 *   3. normalize_likelihoods (src/model/allele_likelihoods.rs:378-508) with
 *      log10_global_read_mismapping_rate as the cap;
 *   4. the keep / remove decision of filter_poorly_modeled_evidence (:925-1041) with the static or
 *      dynamic threshold of :229-239 (computed from the ORIGINAL base qualities, as the reference does).
 * The caller keeps ownership of the evidence lists: `keep[r] == 0` marks reads the reference would move
 * to filtered_evidence_by_sample_index; compaction of the [allele, read] matrix happens when the caller
 * scatters `out` (read-major) into its AlleleLikelihoods.  Per-sample structure does not matter here:
 * every step is per read.
 */
typedef struct phmm_engine_config {
    uint8_t constant_gcp;                                   /* engine.rs:130  (CLI default 10)            */
    uint8_t pcr_error_model;                                /* :61-70  0 None 1 Hostile 2 Aggressive 3 Conservative */
    uint8_t base_quality_score_threshold;                   /* :133    (CLI default 18)                   */
    uint8_t dynamic_read_disqualification;                  /* :134                                       */
    uint8_t symmetrically_normalize_alleles_to_reference;   /* :137                                       */
    uint8_t disable_cap_read_qualities_to_mapq;             /* :138                                       */
    uint8_t reserved[2];
    double log10_global_read_mismapping_rate;               /* :131    cap of normalize_likelihoods       */
    double read_disqualification_scale;                     /* :135                                       */
    double expected_error_rate_per_base;                    /* :136                                       */
} phmm_engine_config;

/*
 *   base_q            ORIGINAL base qualities (read.qual())
 *   ins_q, del_q      BI / BD tags, or NULL for the reference's flat Q45 default (read_utils.rs:23,372-416)
 *   mapq[n_reads]     mapping quality per read (cap_minimum_read_qualities, :438)
 *   region_ref_hap    [n_regions] index INSIDE the region of the reference haplotype, -1 if none; may be
 *                     NULL (only consulted when symmetric normalisation is off)
 *   out               per region row-major [read][hap], NORMALISED log10 likelihoods
 *   keep[n_reads]     1 = evidence kept, 0 = removed as poorly modelled
 * Haplotypes of a region must be distinct (the reference de-duplicates them, haplotype.rs:263-275).
 */
int phmm_engine_compute(phmm_handle *h, const phmm_engine_config *cfg, uint32_t n_regions,
                        const uint32_t *region_read_off, const uint32_t *region_hap_off, const uint32_t *read_off,
                        const uint8_t *read_bases, const uint8_t *base_q, const uint8_t *ins_q,
                        const uint8_t *del_q, const uint8_t *mapq, const uint32_t *hap_off,
                        const uint8_t *hap_bases, const int32_t *region_ref_hap, const uint64_t *out_off,
                        double *out, uint8_t *keep);

/* phmm_engine_compute through the shared, thread-safe queue of phmm_submit (same rules: every array stays caller-owned
 * until phmm_wait(ticket) has returned; phmm_wait is the one above).  Engine-level submissions share a flush when their
 * configurations are equal and the same optional arrays (ins_q / del_q, region_ref_hap) are present; plain and
 * engine-level submissions on one handle are flushed separately, in submission order. */
int phmm_engine_submit(phmm_handle *h, const phmm_engine_config *cfg, uint32_t n_regions,
                       const uint32_t *region_read_off, const uint32_t *region_hap_off, const uint32_t *read_off,
                       const uint8_t *read_bases, const uint8_t *base_q, const uint8_t *ins_q,
                       const uint8_t *del_q, const uint8_t *mapq, const uint32_t *hap_off,
                       const uint8_t *hap_bases, const int32_t *region_ref_hap, const uint64_t *out_off,
                       double *out, uint8_t *keep, uint64_t *ticket);
/* ... and over several engines, one per device, like phmm_compute_multi (contiguous cell-balanced ranges of regions, one
 * pinned host thread per engine, nothing gathered); on failure the message is phmm_last_error(handles[0]). */
int phmm_engine_compute_multi(phmm_handle *const *handles, uint32_t n_handles, const phmm_engine_config *cfg, uint32_t n_regions,
                              const uint32_t *region_read_off, const uint32_t *region_hap_off, const uint32_t *read_off,
                              const uint8_t *read_bases, const uint8_t *base_q, const uint8_t *ins_q, const uint8_t *del_q,
                              const uint8_t *mapq, const uint32_t *hap_off, const uint8_t *hap_bases,
                              const int32_t *region_ref_hap, const uint64_t *out_off, double *out, uint8_t *keep);

/*
 * Smith-Waterman alignment: SmithWatermanAligner::align of the reference
 * (src/smith_waterman/smith_waterman_aligner.rs:47-107 dispatch and exact-substring shortcut, :124-271 calculate_matrix,
 * :273-443 calculate_cigar) for a batch of (reference, alternate) pairs under one parameter set and one overhang
 * strategy -- what each of its call sites has in hand (read -> best haplotype: src/reads/alignment_utils.rs:40-70 via
 * src/assembly/assembly_based_caller_utils.rs:208-246; haplotype -> reference: src/reads/cigar_utils.rs:358-405).
 * Matrix, backtrack and CIGAR assembly all run on the device; the arithmetic is i32 and every tie rule is the
 * reference's, so CIGAR and offset EQUAL the reference's scalar arm (which its own tests assert equal to the vector
 * arm, tests/smith_waterman_aligner_unit_tests.rs:999-1103).
 *
 *   ref_off / alt_off [n+1]   byte offsets of each pair's reference / alternate sequence; what is aligned must be non-empty
 *                             (the reference asserts, :65-68).  Any lengths: up to ~8 000 bases everything of an alignment
 *                             lives in LDS, beyond that its bottom row and strip edges move to device memory (the two
 *                             sequences themselves must fit LDS together: ~80 000 bases each)
 *   params                    gkl::smithwaterman::Parameters::new(match, mismatch, gap open, gap extend).  While
 *                             max |weight| x (longest ref + longest alt + 2) stays below 1e8 -- the range in which the
 *                             reference's clamp at -1e8 (:31) cannot act -- scores travel times four with the winning
 *                             candidate in their low bits; beyond that a wide instance carries them as they are and applies
 *                             the clamp; from 1e9 on, where the reference's own 32-bit sums overflow, PHMM_ERR_INVALID_ARG
 *   overhang_strategy         PHMM_SW_* below == gkl::smithwaterman::OverhangStrategy
 *   cigar_off [n+1]           element offsets into `cigar`: alignment a may use cigar_off[a+1] - cigar_off[a] elements
 *                             (ref_len + alt_len + 3 always suffices; real CIGARs have a handful)
 *   cigar                     elements in BAM encoding, (length << 4) | op with M = 0, I = 1, D = 2, S = 4
 *   n_cigar [n]               elements of each CIGAR; if one exceeds its slot the call returns
 *                             PHMM_ERR_CIGAR_CAPACITY, every other alignment is valid and n_cigar tells the size to retry with
 *   alignment_offset [n]      SmithWatermanAlignmentResult::alignment_offset
 */
#define PHMM_SW_SOFTCLIP 0
#define PHMM_SW_INDEL 1
#define PHMM_SW_LEADING_INDEL 2
#define PHMM_SW_IGNORE 3
typedef struct phmm_sw_parameters {
    int32_t match_value, mismatch_penalty, gap_open_penalty, gap_extend_penalty;
} phmm_sw_parameters;
int phmm_sw_align(phmm_handle *h, uint32_t n_alignments, const uint32_t *ref_off, const uint8_t *ref_bases,
                  const uint32_t *alt_off, const uint8_t *alt_bases, const phmm_sw_parameters *params,
                  int overhang_strategy, const uint64_t *cigar_off, uint32_t *cigar, uint32_t *n_cigar,
                  int32_t *alignment_offset);

/*
 * The same with shared references: alignment a pairs alternate sequence a with reference ref_index[a] -- reads against
 * the few haplotypes of their region, which then cross the bus once instead of once per read.  ref_index[a] ==
 * PHMM_SW_NO_REFERENCE skips the alignment (n_cigar 0, offset 0).  ref_off has n_references + 1 entries.
 */
#define PHMM_SW_NO_REFERENCE 0xffffffffu
int phmm_sw_align_indexed(phmm_handle *h, uint32_t n_references, const uint32_t *ref_off, const uint8_t *ref_bases,
                          uint32_t n_alignments, const uint32_t *ref_index, const uint32_t *alt_off,
                          const uint8_t *alt_bases, const phmm_sw_parameters *params, int overhang_strategy,
                          const uint64_t *cigar_off, uint32_t *cigar, uint32_t *n_cigar, int32_t *alignment_offset);

/*
 * Best allele per read, ties broken by priority: AlleleLikelihoods::best_alleles_breaking_ties_main
 * (src/model/allele_likelihoods.rs:1043-1095) = search_best_allele (:457-554, can_be_reference = true) + BestAllele::new
 * (:1142-1160) for every read of n_regions regions -- the first step of realign_reads_to_their_best_haplotype
 * (src/assembly/assembly_based_caller_utils.rs:208-246) and of the reference's read-allele maps.
 *   likelihoods        per region row-major [read][hap] at out_off[g]: what phmm_engine_compute / phmm_compute return
 *   keep [n_reads]     or NULL: 0 = evidence removed by filter_poorly_modeled_evidence, no best allele (-1)
 *   hap_priority       [n_haps] one i32 per haplotype (haplotype_alignment_tiebreaking_priority, :187-195: is_ref +
 *                      1 - cigar elements; reference_tiebreaking_priority, :197-199), or NULL: no tie breaking
 *   informative_threshold   LOG_10_INFORMATIVE_THRESHOLD = 0.2 (:17) for log10 likelihoods
 *   best_allele [n_reads]   index inside the region, -1 where there is none; likelihood / confidence as BestAllele
 *                      holds them (BestAllele::is_informative: confidence > threshold)
 */
int phmm_best_alleles(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off, const uint32_t *region_hap_off,
                      const uint64_t *out_off, const double *likelihoods, const uint8_t *keep, const int32_t *hap_priority,
                      double informative_threshold, int32_t *best_allele, double *likelihood, double *confidence);

/*
 * Both steps of realign_reads_to_their_best_haplotype that are arithmetic, in one call: the best allele of every read
 * (as phmm_best_alleles) and the read's Smith-Waterman alignment to that haplotype (as phmm_sw_align_indexed; the
 * reference: SoftClip, ALIGNMENT_TO_BEST_HAPLOTYPE_SW_PARAMETERS, src/reads/alignment_utils.rs:40-70).  The index never
 * leaves the device.  `read_bases` are the reads WITHOUT their soft clips (the caller hard-clips them, :47-50); reads
 * without a best allele get n_cigar 0.  Projecting the read -> haplotype CIGAR onto the reference (:83-140) stays with
 * the caller.
 */
int phmm_realign_to_best(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off, const uint32_t *region_hap_off,
                         const uint32_t *read_off, const uint8_t *read_bases, const uint32_t *hap_off,
                         const uint8_t *hap_bases, const uint64_t *out_off, const double *likelihoods, const uint8_t *keep,
                         const int32_t *hap_priority, double informative_threshold, const phmm_sw_parameters *params,
                         int overhang_strategy, const uint64_t *cigar_off, uint32_t *cigar, uint32_t *n_cigar,
                         int32_t *alignment_offset, int32_t *best_allele, double *likelihood, double *confidence);

/*
 * The rest of AlignmentUtils::create_read_aligned_to_ref (src/reads/alignment_utils.rs:40-165), for every read of n_regions
 * regions: the read -> haplotype alignment phmm_realign_to_best returned is projected onto the reference through the
 * haplotype's own CIGAR -- CigarBuilder clean-up (src/reads/cigar_builder.rs), get_consolidated_padded_cigar(1000)
 * (src/haplotype/haplotype.rs:248-256), read_start_on_reference_haplotype (:283-311), trim_cigar_by_bases (:321-386),
 * apply_cigar_to_cigar (:240-281), left_align_indels against the reference haplotype (:425-566), the clips of the read's
 * original CIGAR put back (:173-213) and the length check (:151-161) -- one lane per read on the device.
 *   read_off / read_bases     the reads minus their soft clips (what was aligned)
 *   region_ref_hap [n_regions]          index INSIDE the region of the reference haplotype (left-alignment reads its bases)
 *   region_reference_start [n_regions]  padded_reference_loc.get_start()
 *   hap_cigar_off [n_haps+1], hap_cigar   Haplotype::cigar of every haplotype, BAM-encoded elements
 *   hap_start_wrt_ref [n_haps]          Haplotype::alignment_start_hap_wrt_ref
 *   best_allele, sw_cigar_off / sw_cigar / n_sw_cigar / sw_offset   as phmm_realign_to_best filled them
 *   orig_cigar_off [n_reads+1], orig_cigar   the reads' CIGARs before realignment (only their clips are used)
 *   out_cigar_off [n_reads+1]           element offsets into out_cigar (sw elements + haplotype elements + clips + 4 suffices)
 *   status [n_reads]   PHMM_PROJECT_REALIGNED: new_pos / out_cigar / n_out_cigar are the read's new alignment;
 *                      PHMM_PROJECT_UNCHANGED: no best allele or alignment_offset == -1, the read stays as it is (:60-63);
 *                      negative: the reference panics or returns Err for this read (-1 ... -4 CigarBuilder errors in the
 *                      order of cigar_builder.rs, -5 an assert such as "Read goes past end of reference")
 * Returns PHMM_ERR_CIGAR_CAPACITY when an output slot is too small (n_out_cigar holds the sizes).  Of out_cigar only the
 * elements reported are written: the words of a slot behind them, and the slots of reads that are not realigned, stay.
 */
#define PHMM_PROJECT_REALIGNED 0
#define PHMM_PROJECT_UNCHANGED 1
int phmm_project_to_reference(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off, const uint32_t *region_hap_off,
                              const uint32_t *read_off, const uint8_t *read_bases, const uint32_t *hap_off,
                              const uint8_t *hap_bases, const int32_t *region_ref_hap, const uint64_t *region_reference_start,
                              const uint32_t *hap_cigar_off, const uint32_t *hap_cigar, const uint32_t *hap_start_wrt_ref,
                              const int32_t *best_allele, const uint64_t *sw_cigar_off, const uint32_t *sw_cigar,
                              const uint32_t *n_sw_cigar, const int32_t *sw_offset, const uint32_t *orig_cigar_off,
                              const uint32_t *orig_cigar, const uint64_t *out_cigar_off, uint32_t *out_cigar,
                              uint32_t *n_out_cigar, int64_t *new_pos, int32_t *status);

/*
 * realign_reads_to_their_best_haplotype (src/assembly/assembly_based_caller_utils.rs:208-246) in one call: the best allele
 * of every read (phmm_best_alleles), the read's alignment to that haplotype (phmm_sw_align_indexed) and the alignment
 * projected onto the reference (phmm_project_to_reference) -- the reads and haplotypes cross the bus once, the best
 * alleles and the read -> haplotype alignments never leave the device.  Arguments as in those three calls; per read it
 * returns BestAllele (best_allele / likelihood / confidence) and status / new_pos / out_cigar.  An alignment whose CIGAR
 * outgrows the library's own slots (24 elements) is handled inside (the call runs once more with larger ones).
 */
int phmm_realign_reads(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off, const uint32_t *region_hap_off,
                       const uint32_t *read_off, const uint8_t *read_bases, const uint32_t *hap_off, const uint8_t *hap_bases,
                       const uint64_t *out_off, const double *likelihoods, const uint8_t *keep, const int32_t *hap_priority,
                       double informative_threshold, const phmm_sw_parameters *params, int overhang_strategy,
                       const int32_t *region_ref_hap, const uint64_t *region_reference_start, const uint32_t *hap_cigar_off,
                       const uint32_t *hap_cigar, const uint32_t *hap_start_wrt_ref, const uint32_t *orig_cigar_off,
                       const uint32_t *orig_cigar, const uint64_t *out_cigar_off, uint32_t *out_cigar, uint32_t *n_out_cigar,
                       int64_t *new_pos, int32_t *status, int32_t *best_allele, double *likelihood, double *confidence);

/*
 * One call per region for the whole arithmetic path: what the reference does between
 * PairHMMLikelihoodCalculationEngine::compute_read_likelihoods and AssemblyBasedCallerUtils::
 * realign_reads_to_their_best_haplotype (src/haplotype/haplotype_caller_engine.rs:1311-1357 -- nothing lies between the
 * two but an early return when only one allele is left) in ONE enqueue on one stream:
 *   pre-step (phmm_engine_compute 1.) -> PairHMM forward kernels -> the exact pass below -600 -> normalize_likelihoods +
 *   filter_poorly_modeled_evidence -> best allele per read (phmm_best_alleles) -> the read's Smith-Waterman alignment to
 *   that haplotype -> its projection onto the reference (phmm_project_to_reference).
 * The likelihood matrix, the keep flags, the best alleles and the read -> haplotype alignments never leave the device
 * between the steps; the reads and haplotypes cross the bus once.  Returns what phmm_engine_compute and phmm_realign_reads
 * return together, and equals them field by field (`keep` of the first feeding the second).
 *
 *   cfg / region arrays / read arrays / haplotype arrays / out_off / out / keep     as phmm_engine_compute
 *   read_soft_clip [2 n_reads] or NULL   (leading, trailing) bases of each read that are soft clips: the reference aligns the
 *                      read minus its soft clips (src/reads/alignment_utils.rs:47-50) while the PairHMM sees what
 *                      modify_read_qualities leaves (engine.rs:352-423: all of it with modify_soft_clipped_bases, else the
 *                      clipped read -- then there is nothing to clip here: NULL)
 *   region_ref_hap     REQUIRED here for every region with reads and haplotypes (left-alignment reads the reference haplotype)
 *   rcfg               Smith-Waterman parameters + overhang strategy (the reference: ALIGNMENT_TO_BEST_HAPLOTYPE_SW_PARAMETERS,
 *                      SoftClip), LOG_10_INFORMATIVE_THRESHOLD, flags
 *   hap_priority ... out_cigar_off, best_allele ... status                          as phmm_realign_reads
 * PHMM_REGION_SKIP_SINGLE_ALLELE: a region with exactly one haplotype is not realigned (the reference returns before it
 * gets there, haplotype_caller_engine.rs:1339-1345): its reads keep status PHMM_PROJECT_UNCHANGED, BestAllele is still filled.
 * Any number of regions per call; large calls are pipelined in chunks of regions like phmm_engine_compute.
 *
 * phmm_region_submit is the same call through the shared, thread-safe queue of phmm_submit (phmm_wait is the one above;
 * submissions with equal configurations and the same optional arrays share a flush).
 */
#define PHMM_REGION_SKIP_SINGLE_ALLELE 1u
typedef struct phmm_realign_config {
    phmm_sw_parameters sw_parameters;   /* cigar_utils.rs:22 ALIGNMENT_TO_BEST_HAPLOTYPE_SW_PARAMETERS = (10, -15, -30, -5) */
    int32_t overhang_strategy;          /* PHMM_SW_SOFTCLIP at the reference's call site (alignment_utils.rs:58) */
    uint32_t flags;                     /* PHMM_REGION_* */
    double informative_threshold;       /* LOG_10_INFORMATIVE_THRESHOLD = 0.2 (allele_likelihoods.rs:17) */
} phmm_realign_config;
int phmm_region_compute(phmm_handle *h, const phmm_engine_config *cfg, const phmm_realign_config *rcfg, uint32_t n_regions,
                        const uint32_t *region_read_off, const uint32_t *region_hap_off, const uint32_t *read_off,
                        const uint8_t *read_bases, const uint8_t *base_q, const uint8_t *ins_q, const uint8_t *del_q,
                        const uint8_t *mapq, const uint32_t *read_soft_clip, const uint32_t *hap_off, const uint8_t *hap_bases,
                        const int32_t *region_ref_hap, const uint64_t *out_off, const int32_t *hap_priority,
                        const uint64_t *region_reference_start, const uint32_t *hap_cigar_off, const uint32_t *hap_cigar,
                        const uint32_t *hap_start_wrt_ref, const uint32_t *orig_cigar_off, const uint32_t *orig_cigar,
                        const uint64_t *out_cigar_off, double *out, uint8_t *keep, int32_t *best_allele, double *likelihood,
                        double *confidence, uint32_t *out_cigar, uint32_t *n_out_cigar, int64_t *new_pos, int32_t *status);
int phmm_region_submit(phmm_handle *h, const phmm_engine_config *cfg, const phmm_realign_config *rcfg, uint32_t n_regions,
                       const uint32_t *region_read_off, const uint32_t *region_hap_off, const uint32_t *read_off,
                       const uint8_t *read_bases, const uint8_t *base_q, const uint8_t *ins_q, const uint8_t *del_q,
                       const uint8_t *mapq, const uint32_t *read_soft_clip, const uint32_t *hap_off, const uint8_t *hap_bases,
                       const int32_t *region_ref_hap, const uint64_t *out_off, const int32_t *hap_priority,
                       const uint64_t *region_reference_start, const uint32_t *hap_cigar_off, const uint32_t *hap_cigar,
                       const uint32_t *hap_start_wrt_ref, const uint32_t *orig_cigar_off, const uint32_t *orig_cigar,
                       const uint64_t *out_cigar_off, double *out, uint8_t *keep, int32_t *best_allele, double *likelihood,
                       double *confidence, uint32_t *out_cigar, uint32_t *n_out_cigar, int64_t *new_pos, int32_t *status,
                       uint64_t *ticket);
/* ... and over several engines, normally one per device, like phmm_compute_multi: whole regions in contiguous ranges
 * balanced by cells (phmm_split_regions), every engine on a host thread of its own next to its GPU, each range staged
 * straight from the caller's arrays, results where phmm_region_compute would put them; the arguments are checked once
 * for the whole call; on failure the message is phmm_last_error(handles[0]).  (The reference reaches several devices
 * through its rayon workers instead -- one shared handle per device, phmm_region_submit, integration/hip_backend.rs --
 * which tools/threads_bench TB_DEVICES=n imitates; this entry point is for callers that hold many regions at once.) */
int phmm_region_compute_multi(phmm_handle *const *handles, uint32_t n_handles, const phmm_engine_config *cfg,
                              const phmm_realign_config *rcfg, uint32_t n_regions, const uint32_t *region_read_off,
                              const uint32_t *region_hap_off, const uint32_t *read_off, const uint8_t *read_bases,
                              const uint8_t *base_q, const uint8_t *ins_q, const uint8_t *del_q, const uint8_t *mapq,
                              const uint32_t *read_soft_clip, const uint32_t *hap_off, const uint8_t *hap_bases,
                              const int32_t *region_ref_hap, const uint64_t *out_off, const int32_t *hap_priority,
                              const uint64_t *region_reference_start, const uint32_t *hap_cigar_off, const uint32_t *hap_cigar,
                              const uint32_t *hap_start_wrt_ref, const uint32_t *orig_cigar_off, const uint32_t *orig_cigar,
                              const uint64_t *out_cigar_off, double *out, uint8_t *keep, int32_t *best_allele, double *likelihood,
                              double *confidence, uint32_t *out_cigar, uint32_t *n_out_cigar, int64_t *new_pos, int32_t *status);

/*
 * CigarUtils::calculate_cigar (src/reads/cigar_utils.rs:358-457) for n (reference, haplotype) pairs: the haplotype's CIGAR
 * against the reference -- the two shortcuts (empty haplotype: one D; equal lengths and at most two mismatches: one M),
 * otherwise Smith-Waterman between the sequences padded with "NNNNNNNNNN" on both sides (as phmm_sw_align; the reference's
 * callers use NEW_SW_PARAMETERS and OverhangStrategy::InDel or SoftClip), the padding trimmed off, indels left-aligned,
 * the leading / trailing deletions kept.  Empty sequences are allowed here.
 *   status [n]   0: cigar / n_cigar hold the result; 1: None (is_s_w_failure, :469-487); negative: the reference panics
 * Returns PHMM_ERR_CIGAR_CAPACITY when a slot is too small (n_cigar holds the sizes; ref + alt elements + 2 always suffice).
 */
int phmm_calculate_cigar(phmm_handle *h, uint32_t n, const uint32_t *ref_off, const uint8_t *ref_bases, const uint32_t *alt_off,
                         const uint8_t *alt_bases, const phmm_sw_parameters *params, int overhang_strategy,
                         const uint64_t *cigar_off, uint32_t *cigar, uint32_t *n_cigar, int32_t *status);

/*
 * Per-event genotype likelihoods: the last arithmetic step of the reference's call_region,
 * genotyping_engine.assign_genotype_likelihoods (src/haplotype/haplotype_caller_engine.rs:1379), for many regions in ONE
 * call, on the likelihood matrices phmm_engine_compute / phmm_region_compute return.  For every event e and sample s:
 *   reads used      the reads of e's region with read_sample == s, keep != 0, and Locatable::overlaps with the event window
 *                   as self (src/utils/simple_interval.rs:298-307, all three clauses incl. CoordMath::encloses) -- the
 *                   genotyping predicate of retain_evidence (haplotype_caller_genotyping_engine.rs:759-768), in region order
 *   marginal        M[a][r] = max over haplotypes h with map[h] == a of L[r][h], from -inf (AlleleLikelihoods::marginalize,
 *                   src/model/allele_likelihoods.rs:633-740): an allele no haplotype maps to stays -inf
 *   genotypes       the reference's canonical index order (build_allele_first_genotype_offset_table, allele_heap_to_index:
 *                   genotype_likelihood_calculators.rs:180-224, genotype_likelihood_calculator.rs:273-295); diploid
 *                   0/0, 0/1, 1/1, 0/2, 1/2, 2/2, ...; G_e = phmm_genotype_count(ploidy, A_e) <= 1 024 (the reference's
 *                   max_genotype_count_to_enumerate, haplotype_caller_genotyping_engine.rs:66)
 *   GL              GenotypeLikelihoodCalculator::genotype_likelihoods (genotype_likelihood_calculator.rs:308-580): per read the
 *                   one- / two- / many-component term with the JacobianLogTable sums (src/utils/math_utils.rs:314-370),
 *                   summed over the used reads in order from 0.0, minus n_used * log10(ploidy)
 *   PL              min(round(-10 (GL - max GL)), i32::MAX) with Rust's `as i32` (NaN -> 0): all GLs -inf gives PLs 0
 *                   (Genotype::build_from_likelihoods, src/genotype/genotype_builder.rs:135-152, genotype_likelihoods.rs:55-78)
 * Bit-equal to the reference's operations: no contraction, log10(k) made on the host with std::log10, the host's Jacobian
 * table resident on the device.  The AF calculation is phmm_allele_frequency below; priors, allele trimming and VCF output stay with the caller.
 *   region_read_off / region_hap_off [n_regions+1], out_off [n_regions+1], likelihoods   as phmm_realign_reads
 *   keep [n_reads] or NULL (every read kept)   0: removed by filter_poorly_modeled_evidence (phmm_engine_compute's keep)
 *   read_sample [n_reads]   in [0, n_samples)
 *   read_start / read_end [n_reads]   the read's closed span on the reference after realignment (get_start / get_end,
 *                      src/reads/bird_tool_reads.rs:239-249: end = start + max(reference length - 1, 0))
 *   ploidy             --ploidy (default 2, src/cli.rs:1934-1937), 1..65535
 *   event_region [n_events]; event_allele_off [n_events+1] prefix sums: A_e = off[e+1] - off[e] alleles, allele 0 the reference
 *   event_start / event_end [n_events]   the closed window, already widened by --allele-informative-reads-overlap-margin
 *                      (default 2, haplotype_caller_genotyping_engine.rs:217-229)
 *   event_hap_allele   per event in order, Nh(region(e)) entries: the haplotype's allele, -1 = none
 *   gl_off [n_events+1]   event e writes n_samples x G_e doubles, sample-major [s][g], at gl + gl_off[e]; pl (or NULL) alike
 *   n_evidence [n_events * n_samples] or NULL   the reads used
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offending event or read): a required array NULL,
 * offsets not monotonic, ploidy 0, G_e > 1 024, A_e == 0, a map entry < -1 or >= A_e, event_region >= n_regions,
 * read_sample >= n_samples, a gl_off slot smaller than n_samples x G_e.  n_events == 0 returns PHMM_OK.  One thread per handle.
 */
uint32_t phmm_genotype_count(uint32_t ploidy, uint32_t n_alleles);  /* host only; 0 if either is 0; saturates at UINT32_MAX */
int phmm_genotype_likelihoods(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off,
                              const uint32_t *region_hap_off, const uint64_t *out_off, const double *likelihoods,
                              const uint8_t *keep, const uint32_t *read_sample, const int64_t *read_start,
                              const int64_t *read_end, uint32_t n_samples, uint32_t ploidy, uint32_t n_events,
                              const uint32_t *event_region, const uint32_t *event_allele_off, const int64_t *event_start,
                              const int64_t *event_end, const int32_t *event_hap_allele, const uint64_t *gl_off, double *gl,
                              int32_t *pl, uint32_t *n_evidence);

/*
 * The allele-frequency calculation per event: the arithmetic of the reference's GenotypingEngine::calculate_genotypes
 * (src/genotype/genotyping_engine.rs:80-197) on the PLs phmm_genotype_likelihoods returns, in the same layout, for many
 * events in ONE call -- what the haplotype caller does per event (haplotype_caller_genotyping_engine.rs:297) and the
 * activity profile per reference position (haplotype_caller_engine.rs:1060-1085: alleles N / <FAKE_ALT>, ploidy + 1 PLs).
 *   EM loop         AlleleFrequencyCalculator::calculate (src/model/allele_frequency_calculator.rs:198-379): from the flat
 *                   -log10(A_e), per sample the normalised log10 posteriors of all G_e genotypes (log10 combination count +
 *                   PL / -10 + sum of count x log10 frequency, normalised by MathUtils::log10_sum_log10), the effective allele
 *                   counts summed over samples, the Dirichlet mean weights of prior + counts, until max |Delta count| <= 0.01
 *   prior class     per allele (:205-217): the reference -> ref_pseudo_count; allele_length == the reference's -> SNP; any
 *                   other length -> indel (so <FAKE_ALT>, length 0, against N is an indel)
 *   P(no variant)   the sum over samples of posterior(0/0); with a '*' allele, of min(0, log10_sum_log10) over the genotypes
 *                   made of the reference and '*' alone (:255-300, :381-403)
 *   P(absent)       per alt allele, the sum over samples of min(0, log10_sum_log10) over the genotypes without it (:309-343);
 *                   with A_e == 2 and no '*', P(no variant) itself (:305-307, :348-350)
 *   mle_count       the final effective counts rounded half away from zero (:352-355), the reference's included
 *   allele_flags    PLAUSIBLE: log10_p_absent + 1e-10 < -0.1 stand_min_conf (allele_frequency_calculator_result.rs:115-122);
 *                   OUTPUT: (PLAUSIBLE or the lone alt is <NON_REF>) and not '*' (calculate_output_allele_subset, :390-449)
 *   qual            -10 log10_confidence + 0.0: log10_p_no_variant, or log10_p_variant_present when the site is MONOMORPHIC
 *                   (no alt that is PLAUSIBLE and not '*')
 *   flags           CALLED: calculate_genotypes returns Some (:161-180 with no given alleles); LOW_QUAL: qual < stand_min_conf;
 *                   MONOMORPHIC; TOO_MANY_ALLELES: A_e > 50 (has_too_many_alternative_alleles), nothing computed, not called;
 *                   NOT_CONVERGED: the EM loop met the device's cap of 10 000 iterations (the reference has none)
 * The device assumes what a caller without deletion state and without given alleles has: no event is covered by an upstream
 * deletion (record_deletions :185, is_vc_covered_by_deletion :451), no allele is forced.  A caller with that state sets its
 * covered events' outputs aside (every alt is then spurious: nothing is output and the site is MONOMORPHIC, so QUAL comes
 * from log10_p_variant_present) and adds its forced alleles to those with OUTPUT.  n_samples == 0: no event is called.
 * Not bit-equal: pow / log10 inside the loop are the device's (ocml) and the sums run in a fixed order of their own; results
 * agree with the reference's operations to about 1e-13 relative and are bit-identical from run to run and whatever the batch.
 *   event_allele_off [n_events+1]   A_e = off[e+1] - off[e] alleles, allele 0 the reference; 2 <= A_e
 *   allele_length [off[n]]          Allele::length() (0 for a symbolic allele)
 *   allele_kind [off[n]] or NULL    PHMM_AF_KIND_*; allele 0 plain, at most one '*'; NULL: every allele plain
 *   pl_off [n_events+1], pl         as phmm_genotype_likelihoods' gl_off / pl: n_samples x G_e PLs, sample-major [s][g]
 *   *_pseudo_count                  AlleleFrequencyCalculator::new (make_calculator :53-75: ref = snp_het / het_stdev^2,
 *                                   snp = snp_het x ref, indel = indel_het x ref)
 *   stand_min_conf                  --standard-min-confidence-threshold-for-calling
 *   log10_p_no_variant, log10_p_variant_present (log10_one_minus_pow10 of the former), qual, flags [n_events];
 *   iterations [n_events] or NULL   EM iterations taken
 *   log10_p_absent, mle_count [off[n]], allele_flags [off[n]] or NULL: per allele, the reference's slot 0.0 / its count / 0
 * Events not computed (TOO_MANY_ALLELES, or n_samples == 0) get 0 everywhere but in flags.
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offending event): a required array NULL, offsets not
 * monotonic, ploidy 0, A_e < 2, G_e > 1 024 where A_e <= 50, allele 0 not plain, more than one '*' allele, an unknown kind, a
 * pl_off slot smaller than n_samples x G_e.  n_events == 0 returns PHMM_OK.  One thread per handle.
 */
#define PHMM_AF_KIND_PLAIN 0
#define PHMM_AF_KIND_SPAN_DEL 1
#define PHMM_AF_KIND_NON_REF 2
#define PHMM_AF_CALLED 1u
#define PHMM_AF_LOW_QUAL 2u
#define PHMM_AF_MONOMORPHIC 4u
#define PHMM_AF_TOO_MANY_ALLELES 8u
#define PHMM_AF_NOT_CONVERGED 16u
#define PHMM_AF_ALLELE_PLAUSIBLE 1u
#define PHMM_AF_ALLELE_OUTPUT 2u
int phmm_allele_frequency(phmm_handle *h, uint32_t n_events, uint32_t n_samples, uint32_t ploidy,
                          const uint32_t *event_allele_off, const uint32_t *allele_length, const uint8_t *allele_kind,
                          const uint64_t *pl_off, const int32_t *pl, double ref_pseudo_count, double snp_pseudo_count,
                          double indel_pseudo_count, double stand_min_conf, double *log10_p_no_variant,
                          double *log10_p_variant_present, double *log10_p_absent, int64_t *mle_count,
                          uint8_t *allele_flags, double *qual, uint32_t *flags, uint32_t *iterations);

/*
 * Genotype assignment per event and sample: what GenotypingEngine::calculate_genotypes does with the PLs once the output
 * alleles are known (src/genotype/genotyping_engine.rs:199-235), for many events in ONE call, on the PL layout
 * phmm_genotype_likelihoods writes and phmm_allele_frequency reads -- the FORMAT fields PL, GT, GQ (and GP, PG) of the call,
 * and the sample_called argument of phmm_annotate_events, so the three calls chain without a host step.  Per event e with
 * C_e call alleles and G'_e = phmm_genotype_count(ploidy, C_e):
 *   index table     AlleleSubsettingUtils::subsetted_pl_indices (src/model/allele_subsetting_utils.rs:310-353): the genotype of
 *                   the call with index g' keeps its allele counts, its alleles become the event's, its index there is the old one
 *   likelihoods     pl / -10.0 of the kept genotypes (Genotype::get_likelihoods -> pls_to_gls, genotype_likelihoods.rs:80-85),
 *                   not scaled: the result of scale_log_space_array_for_numeric_stability is discarded there (:214)
 *   sub_pl          gls_to_pls of them (genotype_likelihoods.rs:55-78; depth = vc.get_dp(), emit_empty_pls = true: always set)
 *   PHMM_GT_USE_PLS (UsePLsToAssign, the reference's default; make_genotype_call, src/model/variant_context.rs:309-361)
 *                   is_informative (:573-575): the sum of the likelihoods in index order < SUM_GL_THRESH_NOCALL = -0.1 (:109);
 *                   if not, GT is a no-call and GQ none (UNINFORMATIVE).  Otherwise the genotype is the first maximum
 *                   (MathUtils::max_element_index, src/utils/math_utils.rs:141-150), GQ = (log10 * -10.0).round() as i32
 *                   (genotype_builder.rs:220-222) of get_gq_log10_from_likelihoods (genotype_likelihoods.rs:87-109: the chosen
 *                   minus the largest other, a `>=` scan; its normalising arm needs a negative difference, which the first
 *                   maximum never gives).  A best genotype with <NON_REF> in it: GT no-call, sub_pl all 0, GQ kept (NON_REF_BEST)
 *   PHMM_GT_USE_POSTERIORS (UsePosteriorProbabilities, :380-438)   the priors of GenotypePriorCalculator::assuming_hw(
 *                   log10_snp_het, log10_indel_het, None).get_log10_priors (src/genotype/genotype_prior_calculator.rs:116-229;
 *                   allele types by length against the reference's, '*' included), posteriors = priors + likelihoods, scaled by
 *                   their maximum; pg = priors * -10, gp = scaled posteriors * -10 (== 0.0 -> 0.0); GT the first maximum, never a
 *                   no-call; GQ from get_gq_log10_from_posteriors (:524-571) in its 0/1, 2, 3 and general arms
 *   log10_p_error_posterior   the QUAL update of --use-posteriors-to-calculate-qual (genotyping_engine.rs:216-235):
 *                   phred_no_variant_posterior_probability (:252-269) over extract_p_no_alt_with_posteriors (:282-326, with a '*'
 *                   in the call it reads posteriors[n] for n in 0..ploidy as written there), times -0.1, through
 *                   log10_one_minus_pow10 when site_monomorphic; NaN where the reference makes no update
 *   type            GenotypeBuilder::determine_type (src/genotype/genotype_builder.rs:399-441); sample_called = 1 iff Het, HomVar
 *                   or HomRef, the predicate of get_depth (src/annotator/variant_annotation.rs:369)
 *   C_e == 1        VariantContext::subset_to_ref_only (variant_context.rs:586-619): GT all 0, no PLs, GQ none, called (REF_ONLY)
 * The AD arm of subset_alleles (:274-291) is dead at this call site (the genotypes come from build_from_likelihoods and have
 * no AD): AD stays phmm_annotate_events'.  The other four assignment methods -- SetToNoCall, SetToNoCallNoAnnotations,
 * BestMatchToOriginal (the original GT is empty here) and DoNotAssignGenotypes -- compute nothing and stay with the caller.
 * The default method is bit-equal to the reference's operations.  The posterior method's exp10 / log10 are the device's (ocml)
 * and its log10_sum_log10 adds in a fixed order of its own: about 1e-13 relative, bit-identical from run to run and whatever the batch.
 *   event_allele_off, pl_off, pl    as phmm_allele_frequency
 *   allele_length [off[n]] or NULL  Allele::length(); required by the posterior method
 *   allele_kind [off[n]] or NULL    PHMM_AF_KIND_*: recognises <NON_REF> (default method) and '*' (the QUAL update); NULL: all plain
 *   call_allele_off [n_events+1], call_allele   as phmm_annotate_events: strictly increasing, entry 0 is 0; an event with an
 *                                   empty list is not called: nothing of it is read and its outputs are 0
 *   method                          PHMM_GT_USE_PLS or PHMM_GT_USE_POSTERIORS
 *   log10_snp_het, log10_indel_het  assuming_hw's arguments (log10 of --snp-heterozygosity / --indel-heterozygosity); posterior method
 *   site_monomorphic [n_events] or NULL (0)   PHMM_AF_MONOMORPHIC of phmm_allele_frequency's flags; posterior method
 *   sub_pl_off [n_events+1]         event e writes n_samples x G'_e values, sample-major [s][g'], at sub_pl / gp / pg +
 *                                   sub_pl_off[e]; nothing with C_e <= 1
 *   gt [n_events x n_samples x ploidy]   indices into the event's call_allele list (0 = the reference), non-decreasing
 *                                   (GenotypeAlleleCounts::as_allele_list); -1: a no-call allele
 *   gq [n_events x n_samples]       -1: none;  log10_gq (or NULL): the value before rounding, NaN where GQ is none
 *   sample_called [n_events x n_samples]   phmm_annotate_events' argument
 *   sample_flags [n_events x n_samples]    PHMM_GT_SAMPLE_*
 *   gp, pg, log10_p_error_posterior [n_events]   posterior method only; NULL (and untouched) otherwise
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offending event): a required array NULL, offsets not
 * monotonic, ploidy 0, A_e < 2, an unknown method, and for an event with a call: G_e > 1 024, call_allele[0] != 0, a call allele
 * >= A_e or not increasing, an unknown kind, a pl_off or sub_pl_off slot too small, <NON_REF> in the call with the posterior
 * method (the reference panics there: calculate_allele_types).  n_events == 0 returns PHMM_OK.  One thread per handle.
 */
#define PHMM_GT_USE_PLS 0u
#define PHMM_GT_USE_POSTERIORS 1u
#define PHMM_GT_SAMPLE_UNINFORMATIVE 1u
#define PHMM_GT_SAMPLE_NON_REF_BEST 2u
#define PHMM_GT_SAMPLE_REF_ONLY 4u
int phmm_assign_genotypes(phmm_handle *h, uint32_t n_events, uint32_t n_samples, uint32_t ploidy,
                          const uint32_t *event_allele_off, const uint32_t *allele_length, const uint8_t *allele_kind,
                          const uint64_t *pl_off, const int32_t *pl, const uint32_t *call_allele_off,
                          const uint32_t *call_allele, uint32_t method, double log10_snp_het, double log10_indel_het,
                          const uint8_t *site_monomorphic, const uint64_t *sub_pl_off, int32_t *sub_pl, int32_t *gt,
                          int32_t *gq, double *log10_gq, uint8_t *sample_called, uint8_t *sample_flags, double *gp, double *pg,
                          double *log10_p_error_posterior);

/*
 * The annotation of called events: what the reference does with the read likelihoods once calculate_genotypes has returned
 * a call -- the marginal onto the alleles of the call and VariantAnnotationEngine::annotate_context over it
 * (src/haplotype/haplotype_caller_genotyping_engine.rs:330-393, :451-489; src/annotator/variant_annotator_engine.rs:32-113;
 * src/annotator/variant_annotation.rs:93-405) -- for the events of many regions in ONE call, on the arrays
 * phmm_genotype_likelihoods reads: the FORMAT fields AD, DP, AF, AC and the INFO fields DP, QD, MQ, BQ.  Per event e with
 * C_e call alleles:
 *   reads used      exactly phmm_genotype_likelihoods' rule (keep, read_sample, Locatable::overlaps with the widened window)
 *   marginal        M[a][r] = max over the haplotypes of allele a, from -inf, then the rows of the call's alleles
 *                   (AlleleLikelihoods::marginalize with the one-to-one subset of :376-384, allele_likelihoods.rs:633-740)
 *   best allele     AlleleLikelihoods::search_best_allele with can_be_reference = true and the priorities 1 for the reference,
 *                   0 otherwise (allele_likelihoods.rs:457-554, :1053-1095, assembly_based_caller_utils.rs:197-199): the first
 *                   maximum, then among the alleles within 0.2 of it the highest priority, the second best looked up again;
 *                   BestAllele::new's confidence (:1142-1160); informative iff confidence > 0.2 (:1163)
 *   ad [s][c]       informative reads of sample s by best allele (DepthPerAlleleBySample, variant_annotation.rs:253-291); with
 *                   C_e <= 1 the reference returns before it sets AD (:250-252): ad, af, ac, dp are 0 and flags has NO_AD
 *   dp [s]          the sum of ad (:115-116);  ac [s]: alleles with ad > 0 (:162-171)
 *   af [s][c]       ad / sum (MathUtils::normalize_sum_to_one, utils/math_utils.rs:402-415): a zero sum gives NaN as there
 *   mq [c], bq [c]  over the informative reads of ALL samples with mapq != 0 (is_usable_read :356-358) by best allele: the element
 *                   at index len / 2 of the sorted values (MathUtils::median, math_utils.rs:41-45), 30 when there are none
 *                   (:188-236).  A read's BQ value is ReadUtils::get_read_base_quality_at_reference_coordinate at event_pos
 *                   (src/reads/read_utils.rs:103-173): None outside [read_start, read_end] or before the soft start; the CIGAR
 *                   walk from the soft start in which soft clips advance the reference position; None inside an element that
 *                   consumes no read bases (D, N, H, P); a read that gives None adds nothing
 *   info_dp         the sum of dp over the samples (GenotypesContext::get_dp, genotype/genotype_builder.rs:502-504)
 *   qd_depth        get_depth (:360-405) over the called samples: the sum of dp where it is not 0, restricted to the samples
 *                   with dp - ad[0] > 0 when there is one; a sample with dp == 0 (or NO_AD) counts its used reads + n_filtered
 *                   (sample_evidence_count after add_evidence, haplotype_caller_genotyping_engine.rs:330-341)
 *   qd              -10 log10_p_error / qd_depth (:317-318), the raw value; flags has QD_JITTER when it is not < 45.0: there the
 *                   reference replaces it by 45 + 3 N(0, 1) from a thread RNG (fix_too_high_qd :416-424), which stays with the
 *                   caller.  NO_QD (qd = 0) when the reference returns None: no log10_p_error, n_samples == 0, depth 0 (:302-315)
 * Integers are exact and the doubles bit-equal to the reference's operations (no contraction); nothing depends on the order
 * in which the device counts the reads.  PL subsetting and GT / GQ are phmm_assign_genotypes above (its sample_called goes in
 * here as it is); reverse_trim_alleles and phasing are phmm_phase_calls below; fix_too_high_qd's draw and the VCF strings stay
 * with the caller.
 *   region_read_off ... event_hap_allele   as phmm_genotype_likelihoods
 *   mapq [n_reads]     as phmm_region_compute takes it
 *   call_allele_off [n_events+1], call_allele   the alleles of the call as indices into the event's alleles, strictly
 *                      increasing, entry 0 being 0 (the reference); from phmm_allele_frequency's PHMM_AF_ALLELE_OUTPUT flags.
 *                      An event with an empty list is not annotated: its dp, ac, info_dp, qd_depth, qd and flags are 0
 *   read_off [n_reads+1], base_q   the qualities of each evidence read;  out_cigar_off [n_reads+1] / out_cigar / n_out_cigar
 *                      its CIGAR as phmm_realign_reads returns it (BAM-encoded; the original one for a read left UNCHANGED);
 *                      read_soft_start [n_reads] (get_soft_start); event_pos [n_events] = vc.loc.start.  These seven and bq are
 *                      given together or are all NULL (BQ is then not computed)
 *   sample_called [n_events x n_samples] or NULL (all)   0: the sample's genotype is a no-call (neither het, hom-var nor hom-ref)
 *   log10_p_error [n_events]   the call's (phmm_allele_frequency's qual / -10); NaN (or the reference's 1.0): it has none
 *   n_filtered [n_events x n_samples] or NULL (0)   reads of per_sample_filtered_read_list that overlap the window
 *   ad, af             n_samples x C_e values, sample-major [s][c], at n_samples * call_allele_off[e];  mq, bq: C_e at call_allele_off[e]
 *   dp, ac [n_events x n_samples];  info_dp, qd_depth, qd, flags [n_events]
 * Limits: A_e <= 1 024 (what phmm_genotype_likelihoods admits at ploidy 1); ploidy and the genotype count play no part here.
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offending event or read): a required array NULL,
 * offsets not monotonic, A_e == 0 or > 1 024, a map entry < -1 or >= A_e, event_region >= n_regions, read_sample >= n_samples,
 * call_allele[0] != 0, a call allele >= A_e or not increasing, the BQ arrays given in part, n_out_cigar beyond its slot.
 * n_events == 0 returns PHMM_OK.  One thread per handle.
 */
#define PHMM_ANN_NO_AD 1u
#define PHMM_ANN_NO_QD 2u
#define PHMM_ANN_QD_JITTER 4u
int phmm_annotate_events(phmm_handle *h, uint32_t n_regions, const uint32_t *region_read_off, const uint32_t *region_hap_off,
                         const uint64_t *out_off, const double *likelihoods, const uint8_t *keep, const uint32_t *read_sample,
                         const int64_t *read_start, const int64_t *read_end, const uint8_t *mapq, uint32_t n_samples,
                         uint32_t n_events, const uint32_t *event_region, const uint32_t *event_allele_off,
                         const int64_t *event_start, const int64_t *event_end, const int32_t *event_hap_allele,
                         const uint32_t *call_allele_off, const uint32_t *call_allele, const uint32_t *read_off,
                         const uint8_t *base_q, const uint64_t *out_cigar_off, const uint32_t *out_cigar,
                         const uint32_t *n_out_cigar, const int64_t *read_soft_start, const int64_t *event_pos,
                         const uint8_t *sample_called, const double *log10_p_error, const uint32_t *n_filtered, int32_t *ad,
                         int32_t *dp, double *af, uint32_t *ac, uint8_t *mq, uint8_t *bq, int32_t *info_dp, int32_t *qd_depth,
                         double *qd, uint32_t *flags);

/*
 * Event discovery: the head of the reference's assign_genotype_likelihoods (src/haplotype/haplotype_caller_genotyping_engine.rs:
 * 125-229), for many regions in ONE call -- what lies between phmm_calculate_cigar and phmm_genotype_likelihoods.  Integer and
 * byte work: every output EQUALS the reference's.  Per region:
 *   1. event maps     EventMap::process_cigar_for_initial_events, add_vc, make_block (src/haplotype/event_map.rs:86-344) per
 *                     haplotype: insertions skipped as first / last element, at ref_pos == 0 or over a base that is not regular
 *                     (BaseUtils::is_regular_base is "ACGTacgt": N is not, lower case is); deletions skipped at ref_pos == 0 or over
 *                     such a base; mismatches of an M / = / X element grouped by max_mnp_distance; S advances the haplotype only;
 *                     events of one start merged into a block (SNP + insertion, SNP + deletion, insertion + deletion, SNP +
 *                     insertion + deletion).  As written, a block keeps the type of the alleles its FIRST event had (make_block
 *                     calls get_type() before it replaces them).  Allele bases are upper-cased (ByteArrayAllele::new)
 *   2. loci           the sorted union of the haplotypes' event starts (:361-408) inside the closed window
 *                     (haplotype_caller_genotyping_engine.rs:148)
 *   3. events there   get_overlapping_events (event_map.rs:429-464; a deletion ending here gives way to an insertion here), the
 *                     first occurrence in haplotype order by (start, alleles) (assembly_based_caller_utils.rs:633-658); an event
 *                     that starts before the locus becomes (reference base, '*') (replace_span_dels, :726-751); with
 *                     include_spanning_events == 0 only the events that start at the locus
 *   4. merged context simple_merge as make_merged_variant_context calls it (src/model/variant_context_utils.rs:379-553, :792-916):
 *                     the longest reference allele, every alt extended by the reference's extra tail ('*' is not), alleles in
 *                     first-seen order behind the reference, the span of the longest context.  The priority sort leaves the
 *                     (haplotype) order as it is; events of one haplotype keep their start order
 *   5. allele map     create_allele_mapper (assembly_based_caller_utils.rs:720-840), every branch: no overlapping event -> the
 *                     reference; an event starting here -> its (extended) alt's index, none (-1) if the set does not hold it; an
 *                     event that started earlier -> '*' if present, else the reference, and stop; spanning off -> reference, stop
 *   6. window         event_start / event_end = the merged span through expand_within_contig(overlap_margin, contig length)
 *                     (src/utils/simple_interval.rs:137-147): what phmm_genotype_likelihoods calls "already widened"
 * Inputs, per region g:
 *   region_ref_off [n_regions+1], ref_bases   the padded reference bases;  region_ref_start = ref_loc.start
 *   region_window_start / _end                the closed active_region_window;  region_contig_length  the contig's length
 *   region_hap_off [n_regions+1]; hap_off [n_haps+1], hap_bases; hap_cigar_off [n_haps+1], hap_cigar (BAM-encoded, as
 *   phmm_calculate_cigar writes and phmm_project_to_reference reads); hap_start_wrt_ref [n_haps]   the haplotypes in order
 *   max_mnp_distance (--max-mnp-distance, default 0), include_spanning_events (not --disable-spanning-event-genotyping),
 *   overlap_margin (--allele-informative-reads-overlap-margin, default 2)
 * Outputs, dense over all regions, regions in order, loci ascending inside a region -- they pass AS THEY ARE into
 * phmm_genotype_likelihoods, phmm_allele_frequency, phmm_assign_genotypes and phmm_annotate_events:
 *   region_event_off [n_regions+1]; region_status [n_regions]
 *   event_region, event_start, event_end, event_loc, vc_start, vc_end (the unwidened span), event_flags   [capacity[0]]
 *   event_allele_off [capacity[0]+1];  event_hap_allele [capacity[3]]: per event Nh(region) entries, -1 = none
 *   allele_length, allele_kind (PHMM_AF_KIND_PLAIN / _SPAN_DEL) [capacity[1]]; allele_bases_off [capacity[1]+1];
 *   allele_bases [capacity[2]]   ('*' is the one byte '*', length 1)
 *   optional (hap_event_off NULL skips all seven): the haplotypes' own event maps, dense in haplotype order --
 *   hap_event_off [n_haps+1]; hap_event_start / _end / _ref_length / _type (PHMM_EV_TYPE_*, the cached type) [capacity[4]];
 *   hap_event_alt_off [capacity[4]+1]; hap_event_alt [capacity[5]].  The event's reference allele is hap_event_ref_length
 *   reference bases from hap_event_start.  A region with a negative status has none.
 * PHMM_EV_HAP_IN_TWO_ALLELES (event_flags): create_allele_mapper pushed some haplotype into two allele lists; event_hap_allele
 * holds the first one and the caller treats the event on the host.  As written the reference stops at the first event that
 * starts before the locus and an event map holds one event per start, so no input sets it; the flag stays in the contract.
 * region_status follows the convention above: 0, or negative where the reference panics or returns Err -- then the region has
 * no events and the other regions are unaffected.  The first failing haplotype, in the order the reference meets the failures:
 *   PHMM_EV_STATUS_BAD_OPERATOR   N / P / H in a CIGAR;  PHMM_EV_STATUS_CIGAR_OVERRUN  a CIGAR indexes past the reference or
 *   the haplotype (only where the reference indexes: a deletion at ref_pos == 0 reads nothing);  PHMM_EV_STATUS_BLOCK  an
 *   assertion of make_block (two insertions at one start, ...);  PHMM_EV_STATUS_ALLELES  an event whose alleles are equal once
 *   upper-cased ('a' against 'A': build_event_maps_for_haplotypes returns Err);  PHMM_EV_STATUS_MERGE  simple_merge fails at a
 *   locus: the merged set has no reference allele left (an alt equals the longest reference), or reference alleles of equal
 *   length differ -- which one reference array per region cannot produce.
 * Capacity: capacity[6] = room for events, alleles, allele bytes, map entries, haplotype events, haplotype alt bytes (the last
 * two are read only with hap_event_off).  If one is too small the call returns PHMM_ERR_EVENT_CAPACITY with the six sizes it
 * needs in required[6] and writes nothing else; a call with all capacities 0 is the cheap way to ask.  required is written on
 * success too.  Always sufficient, with E_g = min(reference bases, sum over the haplotypes of bases + CIGAR elements) of region
 * g: events sum E_g; map entries sum E_g Nh_g; alleles sum E_g (1 + 2 Nh_g); allele bytes alleles x (longest reference +
 * longest haplotype + 1); haplotype events and alt bytes: sum over the haplotypes of bases + CIGAR elements.  That bound is a
 * limit, not a way to call: the staging buffer, its pinned mirror and the copy back all have the size of the capacities, so
 * ask first and pass what required holds.
 * Footprint: device memory and pinned host memory for the inputs and for the outputs at their capacities; on the device alone,
 * kept by the handle until phmm_destroy, a workspace of 25 bytes per haplotype base and CIGAR element (plus 200 per haplotype)
 * and 16 bytes per reference base -- about 70 MB for 1 024 regions of 8 haplotypes of 300 bases.
 * Out of scope, the caller's: remove_alt_alleles_if_too_many_genotypes (an event whose phmm_genotype_count(ploidy, A_e) exceeds
 * 1 024 is emitted as it is), given alleles (GGA mode).  Phasing and reverse_trim_alleles are phmm_phase_calls below, which reads
 * the haplotypes' event maps returned here.
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offender): a required array NULL (hap_event_off
 * non-NULL makes the other six map outputs required), offsets that do not start at 0 or are not monotonic, more than PHMM_EVENTS_MAX_REF reference bases or PHMM_EVENTS_MAX_HAPS haplotypes in a region, a contig length of 0,
 * a position from 2^62 on, a base outside "ACGTNacgtnRYKMSWBDHVU" (what the reference's allele constructor takes without
 * making a symbolic allele), a CIGAR element with an operator above 8 or length 0, haplotype bases + CIGAR elements + 8 per
 * haplotype reaching 2^31 in the call (the workspace is indexed in 32 bits).  n_regions == 0 and regions without haplotypes are fine.  Results are identical from run to run and
 * whatever the batch.  One thread per handle.
 */
#define PHMM_EVENTS_MAX_REF 16384u
#define PHMM_EVENTS_MAX_HAPS 512u
#define PHMM_EV_HAP_IN_TWO_ALLELES 1u
#define PHMM_EV_TYPE_SNP 1
#define PHMM_EV_TYPE_MNP 2
#define PHMM_EV_TYPE_INDEL 3
#define PHMM_EV_STATUS_BAD_OPERATOR (-1)
#define PHMM_EV_STATUS_BLOCK (-2)
#define PHMM_EV_STATUS_MERGE (-3)
#define PHMM_EV_STATUS_CIGAR_OVERRUN (-4)
#define PHMM_EV_STATUS_ALLELES (-5)
int phmm_discover_events(phmm_handle *h, uint32_t n_regions, const uint32_t *region_ref_off, const uint8_t *ref_bases,
                         const uint64_t *region_ref_start, const uint64_t *region_window_start, const uint64_t *region_window_end,
                         const uint64_t *region_contig_length, const uint32_t *region_hap_off, const uint32_t *hap_off,
                         const uint8_t *hap_bases, const uint32_t *hap_cigar_off, const uint32_t *hap_cigar,
                         const uint32_t *hap_start_wrt_ref, uint32_t max_mnp_distance, int include_spanning_events,
                         uint32_t overlap_margin, const uint32_t *capacity, uint32_t *required, uint32_t *region_event_off,
                         int32_t *region_status, uint32_t *event_region, uint32_t *event_allele_off, int64_t *event_start,
                         int64_t *event_end, int64_t *event_loc, int64_t *vc_start, int64_t *vc_end, uint32_t *event_flags,
                         int32_t *event_hap_allele, uint32_t *allele_length, uint8_t *allele_kind, uint32_t *allele_bases_off,
                         uint8_t *allele_bases, uint32_t *hap_event_off, int64_t *hap_event_start, int64_t *hap_event_end,
                         uint32_t *hap_event_ref_length, uint32_t *hap_event_alt_off, uint8_t *hap_event_alt,
                         uint32_t *hap_event_type);

/*
 * The activity profile: what the reference computes in front of assembly to decide which stretches of a contig become assembly
 * regions (src/haplotype/haplotype_caller_engine.rs:627-752 update_activity_profile / update_ref_vs_any_results, :754-899
 * parse_record, :908-1107 calculate_activity_probabilities, :1464-1749 alignment_context_creation and what it calls), for many
 * windows, samples and reads in ONE call.  Four stages, all on the device:
 *   1. pileup      one wave per read restates parse_record: a slot per base of an M / = / X element, per base of a D element and
 *                  per I element (ONE entry at the current position; its base is the first inserted base, compared with the
 *                  reference base there), in CIGAR order.  A slot holds counted (quality >= min_base_quality, or a deletion),
 *                  is_alt (:1558-1590, evaluated for counted entries only, so an uncounted base adds no soft clips either), the
 *                  quality (30 for a deletion, :111) and "adds the read's count_high_quality_soft_clips" (qualities > 28, :117).
 *                  Kept as written: next_to_soft_clip_or_indel (:1596-1652) loop for loop; an I element before the window's start
 *                  skips `cig_index += 1`, and the lagging index picks the three CIGAR elements a later deletion inspects
 *                  (:1536-1547); an I element at or past the bounds' end ends the read, a D / M element only itself
 *   2. sums        one lane per position walks the samples in order, a sample's reads in order and a read's slots in CIGAR order:
 *                  genotype_likelihoods[i] += term[is_alt][quality][i] (update_heterozygous_likelihood :1724-1749; the addends
 *                  are host-made with the reference's operations, the middle ones through approximate_log10_sum_log10,
 *                  src/utils/math_utils.rs:314-332), read_counts / ref_depth / non_ref_depth, the soft-clip RunningAverage shared
 *                  by all samples (math_utils.rs:434-477: mean += (obs - mean) / n), gl[i] -= read_counts * log10(ploidy),
 *                  and the PLs of Genotype::build (src/genotype/genotype_builder.rs:104-117, gls_to_pls)
 *   3. is-active   phmm_allele_frequency's kernel on those PLs with one event per position: the reference allele and one
 *                  symbolic alternate of length 0 (the indel prior class), ploidy + 1 genotypes.  is_active_prob =
 *                  CALLED ? (1 - 10^((qual as u8) / -10)) as f32 : 0  (:1080-1085, src/utils/quality_utils.rs:82-104; `as u8`
 *                  saturates, NaN gives 0)
 *   4. band-pass   BandPassActivityProfile::add (src/activity_profile/band_pass_activity_profile.rs:36-105, :210-280;
 *                  src/activity_profile/activity_profile.rs:231-341; activity_profile_state.rs) as a gather.  The Gaussian kernel
 *                  is host-made (make_kernel, determine_filter_size with MIN_PROB_TO_KEEP_IN_FILTER 1e-5, math_utils.rs:383-415)
 *                  and cast to f32 tap by tap; F is the filter size in use.  A state whose (soft-clip mean as f32) >= 6.0 (:75)
 *                  becomes mult = #{i in [-K, K] : 0 <= s + i <= contig length} states, K = min(mean as f32,
 *                  max_prob_propagation as f32) as i64, and as written every one of them re-emits the whole band around the ADDED
 *                  position; any other state has mult = 1.  List entry q = the f32 sum over the sources s ascending, |q - s| <= F,
 *                  prob_s > 0, of prob_s * tap[q - s + F] added mult_s times in a row.  Positions before the profile's first
 *                  state and past the contig length are dropped (the contig length itself is kept, as the reference tests `>`).
 *                  The list is as long as the furthest of: s + 1 for a state without probability, min(s + F, contig length) + 1
 *                  for one with (both from the profile's start)
 * EQUAL to a statement-by-statement restatement: the integers, gl, the soft-clip mean and the band-passed values bit for bit;
 * qual within phmm_allele_frequency's bound with equal flags; is_active_prob is the table value of the device's own
 * `qual as u8`.  Results are identical from run to run and whatever the batch.
 * Per call: ploidy 1..=PHMM_ACTIVITY_MAX_PLOIDY; min_base_quality; the pseudo counts and stand_min_conf of
 * phmm_allele_frequency (the SNP count is part of the contract but no allele here is of its class); max_prob_propagation;
 * max_filter_size (the reference: 50, at most PHMM_ACTIVITY_MAX_FILTER), sigma (17.0), adaptive_filter_size (1); profile_size =
 * the reference's inner_chunk_size: every run of profile_size positions of a window is a BandPassActivityProfile of its own,
 * 0 = one per window.
 * Per window w (the reference's outer chunk): window_start (outer_chunk_location.start), window_len (its size), the contig's
 * length (target_len; the window must end inside it), window_ref_off [n_windows+1] / ref_bases: the reference bases from
 * window_start on, at least window_len of them.
 * Per (window, sample) group g = w * n_samples + s: group_read_off [n_windows * n_samples + 1], its reads after the caller's
 * read_is_filtered IN THE ORDER THE BAM FETCH RETURNED THEM (every sum runs in it); read_pos (0-based) must not decrease
 * inside a group.  Per read: read_cigar_off [n_reads+1] / read_cigar (BAM-encoded), read_off [n_reads+1] / read_bases (ASCII) /
 * read_quals.
 * Outputs; every pointer except window_status may be NULL and is then neither copied back nor written.  With P = the
 * positions of all windows in order (position p of window w at pos_w + p, pos_w = the lengths of the windows before it):
 *   window_status [n_windows]    0, or negative where the reference panics: PHMM_ACT_STATUS_REF_SKIP an N element in a CIGAR of
 *                  the window, PHMM_ACT_STATUS_CIGAR_OVERRUN a CIGAR that consumes more read bases than its read has (the first
 *                  such read decides).  Then every output of the window is 0, its lists are empty, other windows are unaffected
 *   read_counts, ref_depth, non_ref_depth [P * n_samples]   at (pos_w + p) * n_samples + s
 *   gl, pl [P * n_samples * (ploidy + 1)]                   RefVsAnyResult::genotype_likelihoods and the PLs built from them
 *   soft_clip_mean (f64), soft_clip_count, qual, af_flags (PHMM_AF_*), is_active_prob (float) [P]
 *   filter_size [1]; profile_len [profiles]; profile_prob (float) [P + profiles * max_filter_size]: the profiles of all windows
 *                  in order (ceil(window_len / profile_size) per window), profile k's list from P_k + k * max_filter_size, P_k
 *                  the global index of its first position; profile_len[k] entries of it are the state list, the rest is 0
 * Out of scope, the caller's: BAM reading and read_is_filtered, limiting_interval, the depth runs for ANI (they read ref_depth +
 * non_ref_depth).  pop_ready_assembly_regions and the regions' reads are phmm_assembly_regions, which takes profile_prob,
 * profile_len and the read arrays of this call as they are.
 * Footprint: staging for the inputs and the wanted outputs; on the device alone, kept by the handle until phmm_destroy, 6 bytes
 * per pileup slot and about 130 bytes per position plus the outputs not asked for.
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offender): ploidy 0 or above the maximum, no samples,
 * a required array NULL, offsets that do not start at 0 or are not monotonic, fewer reference bases than the window is long, a
 * window that ends past its contig, a position from 2^62 on, read_pos negative or smaller than that of the read before it in its
 * group, a CIGAR element with an operator above 8 or length 0, a sigma the reference's assertions refuse, 2^31 positions.
 * n_windows == 0, windows of length 0 and groups without reads are fine.  One thread per handle.
 *
 * phmm_activity_band_kernel: the host-made kernel alone (filter_size [1], kernel [2 * filter_size + 1] <= 2 * max_filter_size + 1
 * doubles, NULL to ask for the size only); phmm_activity_term_table: the addends of stage 2, [2][256][ploidy + 1].  Both for
 * parity tests.
 */
#define PHMM_ACTIVITY_MAX_PLOIDY 64u
#define PHMM_ACTIVITY_MAX_FILTER 65536u
#define PHMM_ACT_STATUS_REF_SKIP (-1)
#define PHMM_ACT_STATUS_CIGAR_OVERRUN (-2)
int phmm_activity_profile(phmm_handle *h, uint32_t n_windows, uint32_t n_samples, uint32_t ploidy, uint32_t min_base_quality,
                          double ref_pseudo_count, double snp_pseudo_count, double indel_pseudo_count, double stand_min_conf,
                          uint32_t max_prob_propagation, uint32_t max_filter_size, double sigma, int adaptive_filter_size,
                          uint32_t profile_size, const uint64_t *window_start, const uint32_t *window_len,
                          const uint64_t *window_contig_length, const uint32_t *window_ref_off, const uint8_t *ref_bases,
                          const uint32_t *group_read_off, const int64_t *read_pos, const uint32_t *read_cigar_off,
                          const uint32_t *read_cigar, const uint32_t *read_off, const uint8_t *read_bases, const uint8_t *read_quals,
                          int32_t *window_status, uint32_t *read_counts, uint32_t *ref_depth, uint32_t *non_ref_depth, double *gl,
                          int32_t *pl, double *soft_clip_mean, uint32_t *soft_clip_count, double *qual, uint32_t *af_flags,
                          void *is_active_prob, uint32_t *filter_size, void *profile_prob, uint32_t *profile_len);
int phmm_activity_band_kernel(uint32_t max_filter_size, double sigma, int adaptive_filter_size, uint32_t *filter_size, double *kernel);
int phmm_activity_term_table(uint32_t ploidy, double *term);

/*
 * phmm_finalize_reads -- what the reference does to a region's reads before it assembles and again before it genotypes, for
 * many (region, sample) groups in one call: AssemblyBasedCallerUtils::finalize_regions up to its first sort
 * (src/assembly/assembly_based_caller_utils.rs:97-172) with clean_overlapping_read_pairs (:263-289), and
 * AssemblyRegion::trim_with_padded_span's map + filter (src/assembly/assembly_region.rs:341-352).  Restated as written:
 * ReadClipper (src/reads/read_clipper.rs:63-530), ClippingOp::apply_hard_clip_bases / apply_revert_soft_clipped_bases
 * (src/reads/clipping_op.rs:100-139, :201-235), CigarUtils::clip_cigar / revert_soft_clips / alignment_start_shift
 * (src/reads/cigar_utils.rs:149-330), ReadUtils (src/reads/read_utils.rs:103-148, :190-211, :288-364), BirdToolRead::get_start /
 * get_end / get_soft_start (src/reads/bird_tool_reads.rs:76-104, :239-249), FragmentCollection::create
 * (src/utils/fragment_collection.rs:32-76), adjust_quals_of_overlapping_paired_fragments (src/utils/fragment_utils.rs:27-149).
 * Everything runs on the device; a missing kernel is an error, there is no host path.
 *
 * cfg->steps (PHMM_FIN_*): a step that is not set is the identity, and the conditions between the steps stay in every
 * combination -- get_start() <= get_end(), !is_unmapped before the adaptor step, !is_empty && seq_len_from_cigar > 0 before the
 * region step, the final overlap test.  PHMM_FIN_ALL is finalize_regions; PHMM_FIN_REGION alone is trim_with_padded_span.
 *   PHMM_FIN_SOFT_CLIPS     hard_clip_soft_clipped_bases when cfg->dont_use_soft_clipped_bases or the read has no well-defined
 *                           fragment size, else revert_soft_clipped_bases (:124-131)
 *   PHMM_FIN_LOW_QUAL_ENDS  hard_clip_low_qual_ends(cfg->min_tail_quality): the caller passes
 *                           MIN_TAIL_QUALITY_WITH_ERROR_CORRECTION (6) with --error-correct-reads, else
 *                           min-base-quality.saturating_sub(1) (:109-113, :308-309)
 *   PHMM_FIN_ADAPTOR        hard_clip_adaptor_sequence
 *   PHMM_FIN_REGION         hard_clip_to_region(group_span_start, group_span_end)
 *   PHMM_FIN_PAIRS          the base qualities of overlapping mates; cfg->half_of_pcr_snv_qual (the reference: 20,
 *                           fragment_utils.rs:9-14).  Needs mate_index.
 * Per group g (one region, one sample): group_read_off [n_groups+1], group_span_start / group_span_end [n_groups]: the padded
 * span the reference passes (region.get_padded_span(), both ends as the reference holds them).
 * cfg points to a phmm_finalize_config and read_flags to uint16_t [n_reads]; both are declared `const void *` like the float
 * arrays of phmm_activity_profile, so that the prototype keeps to the scalar types every binding of this header knows.
 * Per read: read_pos (0-based), read_flags (BAM flags, uint16_t), read_mapq, read_mpos, read_isize, read_cigar_off [n_reads+1] /
 * read_cigar (BAM-encoded), read_off [n_reads+1] / read_bases / read_quals, mate_index (or the whole array NULL): the
 * call-wide index of the one other read of the same group with the same name, -1 for none -- the caller holds the names, and
 * clipping does not change them.  read_bases is read by PHMM_FIN_PAIRS alone and may be NULL without it.
 * Outputs per read, in input order; every pointer except read_status may be NULL and is then neither written nor copied back
 * (out_cigar needs out_cigar_off and n_out_cigar):
 *   read_status    0, or negative where the reference would panic (PHMM_FIN_STATUS_*); then keep = 0, the other per-read outputs
 *                  are 0 and out_quals is the input's -- a panic of the pair step leaves the outputs of the clip steps as they
 *                  were and sets keep = 0 and the status of both reads.  Nothing else in the call is affected.  Debug-build
 *                  arithmetic decides what panics; a release build of the reference would wrap instead.
 *                    PHMM_FIN_STATUS_CIGAR        a CigarBuilder result the reference unwraps is an Err (clip_cigar, revert_soft_clips)
 *                    PHMM_FIN_STATUS_CLIP_RANGE   the three range panics of clip_by_reference_coordinates
 *                    PHMM_FIN_STATUS_ARITHMETIC   a usize conversion or subtraction that fails: get_soft_start().unwrap() on a
 *                                                 negative value, mpos as usize - 1, read.len() - (stop - start + 1)
 *                    PHMM_FIN_STATUS_PAIR         an unwrap on None, or an index past a read, in the pair step
 *                    PHMM_FIN_STATUS_WORKSPACE    more CIGAR elements than reserved (never with the room the call derives)
 *   keep (u8)      what the reference's filter_map / filter decides (:148-167, assembly_region.rs:351)
 *   new_pos        the read's position; the other outputs describe the read whether it is kept or not
 *   out_unmapped (u8)   set for a read empty_read has touched (it is unmapped, its mate unmapped, mapq 0, no bases, no CIGAR)
 *   clip_first, clip_len   clipping only ever removes bases from the two ends: the result's bases and qualities are the window
 *                  [clip_first, clip_first + clip_len) of the input's.  No base is copied.
 *   out_cigar_off [n_reads+1] (in): where each read's CIGAR goes in out_cigar, with room for the read's elements + 2 (a clip
 *                  splits at most one element per end); out_cigar, n_out_cigar.  Room a read does not use is not written.
 *   unclipped_len  AlignmentUtils::unclipped_read_length (src/reads/alignment_utils.rs:680-694); with read_mapq and the flags
 *                  the caller applies the filters of haplotype_caller_engine.rs:1250-1273 without touching a CIGAR
 *   lead_soft, trail_soft   the soft clip behind the leading hard clips and the one before the trailing hard clips: the pair
 *                  phmm_region_compute takes as read_soft_clip
 *   out_quals      (the layout of read_quals) the input qualities with the pair step's changes; bytes outside a read's window and
 *                  reads not kept are copied unchanged
 * Quirks kept: get_end() of an empty CIGAR is get_start(); clip_read clamps an operation's stop to the current length and skips
 * one whose start is past it; the right-tail scan of clip_low_qual_ends never goes below index 0; a reverted read whose soft
 * start is <= 0 loses 1 - soft_start bases and lands on position 0; hard_clip_to_region clips at ref_start.saturating_sub(1) /
 * ref_stop + 1; hard_clip_both_ends clips the right tail first and empties the read when left > get_end() afterwards;
 * clip_cigar drops a deletion that touches the cut; a read emptied by any step is unmapped from then on and skips the adaptor
 * step; a read that came in flagged unmapped gets the CIGAR 0M from a hard clip; the pair step takes the read with the smaller
 * soft start as the first one and the SECOND of the pair when the soft starts are equal.
 * Pairs: FragmentCollection::create meets the two reads of a pair in the reference's sorted order.  The comparator's keys the
 * device knows decide it, in this order: new_pos, reverse strand, flags, mapq, mpos, clipped length, then the lower input index.
 * The reference compares names before flags -- mates share theirs -- and its unstable sort leaves complete ties open; here the
 * lower index comes first.  A read is a pair candidate by fragment_collection.rs:47-51 evaluated on the clipped read; a candidate
 * whose mate is not a kept candidate is a singleton.
 * Out of scope, the caller's: the two par_sort_unstable calls, soft_clip_low_quality_ends (hidden flag, default off), BI / BD
 * qualities (the reference does not clip them either, clipping_op.rs:233), the error corrector, the MAPQ / mate-contig filter.
 * The output is the same from run to run and whatever else is in the batch (no atomics, one writer per element).
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offender): a required pointer NULL (cfg, the group
 * arrays, the read arrays, read_status, mate_index with PHMM_FIN_PAIRS), unknown step bits, offsets that do not start at 0 or
 * decrease, a CIGAR element with an operator above 8 or length 0, a CIGAR whose read length differs from the read's base count,
 * span_end < span_start, positions from 2^62 on (read_pos negative included; mpos and isize by magnitude), less room in
 * out_cigar_off than a read needs, a mate_index that is out of its group, self-referential or not symmetric.
 * n_groups == 0, empty groups and reads of length 0 are fine.  One thread per handle.
 */
#define PHMM_FIN_SOFT_CLIPS 1u
#define PHMM_FIN_LOW_QUAL_ENDS 2u
#define PHMM_FIN_ADAPTOR 4u
#define PHMM_FIN_REGION 8u
#define PHMM_FIN_PAIRS 16u
#define PHMM_FIN_ALL 31u
#define PHMM_FIN_STATUS_CIGAR (-1)
#define PHMM_FIN_STATUS_CLIP_RANGE (-2)
#define PHMM_FIN_STATUS_ARITHMETIC (-3)
#define PHMM_FIN_STATUS_PAIR (-4)
#define PHMM_FIN_STATUS_WORKSPACE (-5)
typedef struct phmm_finalize_config {
    uint32_t steps;                      /* PHMM_FIN_* */
    uint8_t min_tail_quality;
    uint8_t dont_use_soft_clipped_bases;
    uint8_t half_of_pcr_snv_qual;
    uint8_t reserved;
} phmm_finalize_config;
int phmm_finalize_reads(phmm_handle *h, const void *cfg, uint32_t n_groups, const uint32_t *group_read_off,
                        const uint64_t *group_span_start, const uint64_t *group_span_end, const int64_t *read_pos,
                        const void *read_flags, const uint8_t *read_mapq, const int64_t *read_mpos, const int64_t *read_isize,
                        const uint32_t *read_cigar_off, const uint32_t *read_cigar, const uint32_t *read_off,
                        const uint8_t *read_bases, const uint8_t *read_quals, const int32_t *mate_index,
                        const uint64_t *out_cigar_off, int32_t *read_status, uint8_t *keep, int64_t *new_pos, uint8_t *out_unmapped,
                        uint32_t *clip_first, uint32_t *clip_len, uint32_t *out_cigar, uint32_t *n_out_cigar,
                        uint32_t *unclipped_len, uint32_t *lead_soft, uint32_t *trail_soft, uint8_t *out_quals);

/*
 * phmm_phase_calls -- the tail of the reference's assign_genotype_likelihoods for many regions in ONE call: reverse_trim_alleles
 * as make_annotated_call applies it, the called haplotypes, and physical phasing (phase_calls).  It reads the dense arrays as
 * phmm_discover_events, phmm_annotate_events and phmm_assign_genotypes take and write them, so a caller chains discovery ->
 * likelihoods -> AF -> assignment -> annotation -> phasing without rebuilding anything on the host.  Integers and bytes: every
 * output EQUALS the reference's.  Per region, over its called events (C_e = call_allele_off[e+1] - call_allele_off[e] >= 1) in
 * order:
 *   1. reverse trim   make_annotated_call (src/haplotype/haplotype_caller_genotyping_engine.rs:451-489) trims a call only when
 *                     C_e != A_e.  VariantContextUtils::trim_alleles(vc, false, true) (src/model/variant_context_utils.rs:
 *                     956-1108) over AlignmentUtils::normalize_alleles(seqs, ranges, 0, true) (src/reads/alignment_utils.rs:
 *                     585-675), as written: C_e <= 1, or any allele of length 1 that is not symbolic ('*' is one), leaves the
 *                     call as it is; <NON_REF> is left out of the sequences and kept; all three loops of normalize_alleles run
 *                     (the forward loop decides empty_allele and with it restore_one_base_at_end); the start does not move,
 *                     call_rev_trim bases leave the end of every allele that is not symbolic, call_end = vc_start + len(ref) -
 *                     call_rev_trim - 1.  The trimmed allele is the first length - call_rev_trim bytes: no base is copied.
 *                     PHMM_PH_NO_TRIM in flags: no call is trimmed, phasing sees the alleles as given
 *   2. called haplotypes   (:394-405) allele_mapper.remove(&idx) for idx in 0..C_e.  As written: the map is keyed by the MERGED
 *                     context's allele index and idx is a POSITION in the call's list, so a call that kept alleles {0, 2} of
 *                     three contributes the haplotypes of merged alleles 0 and 1.  Haplotype h is called iff
 *                     0 <= event_hap_allele[e][h] < C_e for some called event e of its region
 *   3. phase_calls    (src/assembly/assembly_based_caller_utils.rs:975-1348)
 *                     construct_haplotype_mapping: a call with exactly one site-specific alternate allele (not the reference,
 *                     not '*', not <NON_REF>) gets S_e = the called haplotypes whose event map holds an event with start ==
 *                     vc_start[e] and an alternate allele equal, byte for byte, to the TRIMMED allele; every other call the empty
 *                     set.  A merged alt that was extended by the reference's tail and not trimmed back matches nothing: as written
 *                     construct_phase_set_mapping: total = |union of S_e|; for i < j with non-empty sets, "together" iff
 *                     (|Si| == |Sj| and Sj within Si) or |Sj| == total, else "apart" iff |Si| + |Sj| == total and Si, Sj disjoint.
 *                     The reference's middle clause of "together" tests call_haplotypes_available_for_phasing, which is created
 *                     empty and only ever retain()ed: it is false for every non-empty Sj and restated as such, not repaired.
 *                     On a related pair: i unmapped and j mapped clears the whole region's mapping and returns
 *                     (PHMM_PH_ABORTED, nothing in the region is phased); both unmapped open group unique_counter, i 0|1 and
 *                     j 0|1 (together) or 1|0 (apart); i mapped and j unmapped: j joins i's group with i's phase or the flipped
 *                     one; both mapped: nothing
 *                     construct_phase_groups / phase_vc: the group's first call in order leads it, PS is its start; every
 *                     genotype of a member becomes phased; its allele list is reversed iff it is Het (determine_type: no no-call
 *                     allele, two different alleles) and alleles[alt_allele_index] (1 for 0|1, 0 for 1|0) is not site-specific;
 *                     && short-circuits, so ploidy 1 never indexes
 * The reference has no test of phase_calls, trim_alleles or normalize_alleles: this restatement is pinned by reading.
 * Inputs:
 *   region_event_off, region_hap_off [n_regions+1]; event_allele_off; event_hap_allele; vc_start; allele_length; allele_kind
 *   (PHMM_AF_KIND_*); allele_bases_off; allele_bases; hap_event_off [n_haps+1]; hap_event_start; hap_event_alt_off;
 *   hap_event_alt       as phmm_discover_events writes them (with its per-haplotype event maps: ascending by start, one per start)
 *   call_allele_off [n_events+1], call_allele   as phmm_annotate_events takes them; an empty list: the event is not called
 *   n_samples, ploidy, gt [n_events x n_samples x ploidy]   phmm_assign_genotypes' gt; gt NULL skips the genotype stage, and
 *                       is_phased and gt_phased must then be NULL too
 *   flags               0 or PHMM_PH_NO_TRIM
 * Outputs, per event unless noted; an event that is not called gets 0, and -1 in call_end, phase_group, phase_leader, phase_set
 * and gt_phased:
 *   call_rev_trim, call_end;  phase_n_haps = |S_e|;  hap_in_call (in event_hap_allele's layout, 1 iff the haplotype is in S_e;
 *   NULL skips it);  phase_group (-1 = unphased, else the reference's unique_counter value within the region);  phase_gt
 *   (PHMM_PH_GT_01 / PHMM_PH_GT_10);  phase_leader (the event index of the group's first call, -1 unphased: its start is PS, its
 *   reference and first alt make the ID string);  phase_set (PS, -1 unphased);  region_alt_haps [n_regions] (total);
 *   region_phase_flags [n_regions] (PHMM_PH_ABORTED);  is_phased [n_events x n_samples];  gt_phased [n_events x n_samples x
 *   ploidy] (gt, reversed where phase_vc reverses).  The strings 0|1, 1|0 and the ID are the caller's to format.
 * Precondition, not checked: a region's haplotypes differ by bases (the reference's HashSet<Haplotype> compares bases; the
 * assembler's result set guarantees it).  Limits: PHMM_EVENTS_MAX_HAPS haplotypes per region (a set is 512 bits); events per
 * region as phmm_discover_events.  Device workspace kept by the handle: 68 bytes per event and 64 per region.
 * The result is the same from run to run and whatever else is in the batch: the one atomic is an OR, every other element has
 * one writer.
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offender): a required array NULL (gt without its two
 * outputs, or they without gt), unknown flag bits, offsets that do not start at 0 or decrease, more than PHMM_EVENTS_MAX_HAPS
 * haplotypes in a region, a call list that does not start with 0, is not strictly increasing or reaches A_e, an unknown kind, a
 * reference allele that is not plain, a call allele that is not symbolic with length 0 or more bases than its slot, ploidy 0
 * with gt given, a gt entry outside [-1, C_e), haplotype events that do not ascend by start.  n_regions == 0, regions without
 * events and regions without haplotypes are fine.  One thread per handle.
 */
#define PHMM_PH_NO_TRIM 1u
#define PHMM_PH_ABORTED 1u
#define PHMM_PH_GT_01 0
#define PHMM_PH_GT_10 1
int phmm_phase_calls(phmm_handle *h, uint32_t n_regions, const uint32_t *region_event_off, const uint32_t *region_hap_off,
                     const uint32_t *event_allele_off, const int32_t *event_hap_allele, const int64_t *vc_start,
                     const uint32_t *allele_length, const uint8_t *allele_kind, const uint32_t *allele_bases_off,
                     const uint8_t *allele_bases, const uint32_t *hap_event_off, const int64_t *hap_event_start,
                     const uint32_t *hap_event_alt_off, const uint8_t *hap_event_alt, const uint32_t *call_allele_off,
                     const uint32_t *call_allele, uint32_t n_samples, uint32_t ploidy, const int32_t *gt, uint32_t flags,
                     uint32_t *call_rev_trim, int64_t *call_end, uint32_t *phase_n_haps, uint8_t *hap_in_call,
                     int32_t *phase_group, uint8_t *phase_gt, int32_t *phase_leader, int64_t *phase_set,
                     uint32_t *region_alt_haps, uint32_t *region_phase_flags, uint8_t *is_phased, int32_t *gt_phased);

/*
 * phmm_assembly_kmers -- what the reference's read-threading assembler decides from k-mers alone, in front of the graph, for
 * many regions and several k in ONE call: the sequences add_read makes of each read, the non-unique k-mers, where each sequence
 * starts threading and which positions it visits, how many k-mers kmer_to_vertex_map will hold, and the verdicts that reject a
 * k before a vertex exists.  The raw graph -- vertices, edges, multiplicities -- is phmm_assembly_graph's, which runs this stage
 * inside; pruning, dangling ends and paths stay the caller's.  Integers and bytes: every output EQUALS the reference's.  R = src/read_threading/read_threading_graph.rs,
 * A = src/read_threading/read_threading_assembler.rs, K = src/assembly/kmer.rs.  Per region and k, as written:
 *   sequences    create_graph (A:924-1089) adds the reference as one sequence (start 0, stop len), then add_read per read
 *                (R:341-390): each maximal run of bases with to_ascii_uppercase(base) != 'N' and qual >= min_base_quality
 *                (R:400-403) of length >= k is a sequence (the whole read, start, stop).  An empty read adds nothing
 *   non-unique   the union over the sequences of determine_non_unique_kmers (R:111-141, R:164-187), whose loop runs over
 *                0 ..= stop - k: from 0, NOT from start.  A run scans the read's prefix in front of it, unusable bases included,
 *                so a k-mer that holds an N or a low-quality base can be in the set.  Kept as written
 *   equality     the reference's Kmer compares a 64-bit SipHash of the bytes and the length (K:73-89, K:154-158), case-sensitive.
 *                This call compares BYTES: two different k-mers that collide in SipHash are equal there and not here
 *   start        set_threading_start_only_at_existing_vertex(!recover_dangling_branches) (A:980) with the default, dangling
 *                branch recovery on: a sequence starts at its first k-mer that is not non-unique (R:239-248).  find_start
 *                (R:569-588): the reference starts at 0; a run searches start .. stop.saturating_sub(k), the bound EXCLUSIVE,
 *                so its last k-mer is never a start.  thread_sequence (R:484-561) returns at once if the WHOLE sequence's
 *                length is <= start_pos + k (a reference of exactly k bases threads nothing), else it visits start_pos ..= stop - k.
 *                The other mode (start only at an existing vertex) depends on the order of threading and is not part of this call
 *   vertex map   track_kmer (R:635-639) enters a k-mer when a vertex is created for it, unless it is non-unique or already
 *                there; extend_chain_by_one (R:700-769) follows an edge or merges into the mapped vertex, the reference-source
 *                k-mer excepted (R:613-618), which gets a fresh vertex that is not entered again.  So the map holds the distinct
 *                k-mers that some sequence visits and that are not non-unique
 *   verdicts     reference shorter than k: a failed result (A:935-938), PHMM_ASM_REF_SHORT, and every other output of that
 *                (k, region) is 0 (ids UINT32_MAX); determine_non_unique_kmers(reference) not empty: PHMM_ASM_REF_NON_UNIQUE
 *                (A:940-956; the caller may allow it, so everything else is still computed); is_low_quality_graph (R:261-263)
 *                n_non_unique * 4 > n_tracked: PHMM_ASM_LOW_COMPLEXITY (pruning touches neither set)
 * Inputs:
 *   region_ref_off [n_regions+1], ref_bases      the regions' reference haplotypes, one behind the other
 *   region_read_off [n_regions+1], read_off [n_reads+1], read_bases, read_quals    the regions' reads in input order
 *   read_first, read_len [n_reads] or both NULL  the read IS bases [read_first, read_first + read_len) of its slot: what
 *                phmm_finalize_reads returns as clip_first / clip_len, so its output feeds this call with no base copied
 *   n_k, k [n_k]   1 <= n_k <= PHMM_ASM_MAX_K_VALUES, 1 <= k <= PHMM_ASM_MAX_K, ascending; the same list for every region
 *   min_base_quality   the reference's default is 10
 * Outputs:
 *   flags, n_sequences, n_non_unique, n_tracked, n_distinct [n_k x n_regions]   PHMM_ASM_REF_* / LOW_COMPLEXITY; the reference
 *                plus the runs of >= k bases (count + 1 of A:1004-1016); the size of the non-unique set; kmer_to_vertex_map.len()
 *                after build_graph_if_necessary; the distinct k-mers over all scanned positions
 *   ref_kmer_flags [n_k x region_ref_off[n_regions]], read_kmer_flags [n_k x read_off[n_reads]]   k-major planes over ref_bases
 *                and read_bases as given, a byte per position p of a sequence.  A position is SCANNED if some
 *                determine_non_unique_kmers loop reaches it: every p <= len - k of the reference, every p <= stop - k of a read
 *                whose last run of >= k bases ends at stop.  PHMM_ASM_KMER_NON_UNIQUE: the k-mer at p is in the region's set;
 *                _THREADED: thread_sequence visits p as part of some run; _THREAD_START: find_start returns p for its run
 *                (for a reference of exactly k bases position 0 has _THREAD_START and not _THREADED); _FIRST: p is the first
 *                occurrence of its bytes among the region's scanned positions, the reference first, then the reads in input
 *                order, positions ascending.  0 where p is not scanned (p + k beyond the read included) and outside a window
 *   ref_kmer_id, read_kmer_id   both NULL (not written) or the same planes as u32: dense ids in the order of _FIRST, equal
 *                bytes equal ids within a (k, region), UINT32_MAX where the position is not scanned: what a host assembler keys
 *                its vertex map with instead of hashing byte slices
 * Limits: PHMM_ASM_MAX_REF_BASES per region's reference, PHMM_ASM_MAX_READ_BASES per read (its window),
 * (reference bases + read bases) x n_k <= PHMM_ASM_MAX_POSITIONS (the workspace is indexed with 32 bits).  Device workspace kept
 * by the handle: 45 bytes per base and k (53 when some sequence is longer than 1 024 bases and its own table leaves LDS), and
 * 10 per base for the prefix hash and the runs.
 * The result is the same from run to run and whatever else is in the batch: which position claims a slot of a table is a
 * race that no output shows; the other atomics are minima, ORs and integer sums.
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offender): n_k outside 1..PHMM_ASM_MAX_K_VALUES; a k
 * outside 1..PHMM_ASM_MAX_K; k not ascending; min_base_quality above 255; read_first without read_len or the reverse; one id
 * plane without the other; a required array NULL; region_ref_off, region_read_off or read_off that does not start at 0 or
 * decreases; a window outside its read; a reference or a read above its limit; bases x n_k above PHMM_ASM_MAX_POSITIONS.
 * n_regions == 0, regions without reads and empty reads are fine.  One thread per handle.  Switch "asm_fingerprint_bits"
 * (tests): the tables' fingerprints keep that many bits, so probing and the byte comparison run on ordinary inputs; the
 * outputs do not change.
 */
#define PHMM_ASM_MAX_K_VALUES 8u
#define PHMM_ASM_MAX_K 255u
#define PHMM_ASM_MAX_REF_BASES 16384u
#define PHMM_ASM_MAX_READ_BASES 16384u
#define PHMM_ASM_MAX_POSITIONS 536870912u
#define PHMM_ASM_REF_SHORT 1u
#define PHMM_ASM_REF_NON_UNIQUE 2u
#define PHMM_ASM_LOW_COMPLEXITY 4u
#define PHMM_ASM_KMER_NON_UNIQUE 1u
#define PHMM_ASM_KMER_THREADED 2u
#define PHMM_ASM_KMER_THREAD_START 4u
#define PHMM_ASM_KMER_FIRST 8u
int phmm_assembly_kmers(phmm_handle *h, uint32_t n_regions, const uint32_t *region_ref_off, const uint8_t *ref_bases,
                        const uint32_t *region_read_off, const uint32_t *read_off, const uint8_t *read_bases,
                        const uint8_t *read_quals, const uint32_t *read_first, const uint32_t *read_len, uint32_t n_k,
                        const uint32_t *k, uint32_t min_base_quality, uint32_t *flags, uint32_t *n_sequences,
                        uint32_t *n_non_unique, uint32_t *n_tracked, uint32_t *n_distinct, uint8_t *ref_kmer_flags,
                        uint8_t *read_kmer_flags, uint32_t *ref_kmer_id, uint32_t *read_kmer_id);

/*
 * phmm_assembly_graph -- the raw read-threading graph per (k, region), exactly as it stands right after
 * build_graph_if_necessary (R:417-477, called at A:1020): before prune_low_weight_chains, the cycle checks and dangling-end
 * recovery, for many regions and several k in ONE call.  It runs phmm_assembly_kmers' stage inside and builds on its state.
 * Integers and bytes: every output EQUALS the reference's, petgraph's NodeIndex and EdgeIndex included.  R, A, K as above,
 * E = src/graphs/multi_sample_edge.rs.  Default modes only: start_threading_only_at_existing_vertex = false,
 * increase_counts_through_branches = false, INCREASE_COUNTS_BACKWARDS = true, count = 1 per sequence.  LEFT OUT, the
 * caller's: the other settings of those modes, and everything behind the raw graph (pruning, cycles, dangling ends, paths).
 * Kmer equality is of bytes, not of SipHash values, as in phmm_assembly_kmers.  As written:
 *   order        the reference is threaded first, then the sample groups in order of the first read THAT YIELDS A SEQUENCE AT
 *                THAT K (pending.entry, R:328, a LinkedHashMap), reads in input order inside a group, a read's runs in order.
 *                The group order can differ between two k of one region
 *   vertices     thread_sequence (R:484-561): the start's vertex is the map's or a new one (R:597-605); extend_chain_by_one
 *                (R:700-769) follows the out-edge whose target has the next base as its suffix, else merges into the map's
 *                vertex for the k-mer -- never for the reference-source k-mer (R:613-618) -- else creates one; a non-unique
 *                k-mer is never in the map (R:635-639), so it gets a vertex per (vertex before it, last base)
 *   edges        one per (source, target); is_ref is the creating sequence's; multiplicity counts the traversals (the inherent
 *                MultiSampleEdge::inc_multiplicity, E:89-92) plus the backward walk's
 *   backward     increase_counts_in_matched_kmers (R:641-687) from the start vertex with offset k - 2 (none for k = 1): while
 *                the vertex has exactly ONE in-edge at that moment and the edge's source has the suffix sequence[offset], the
 *                edge gains 1 and the walk goes on from the source with offset - 1.  sequence is the WHOLE sequence (R:504), so
 *                the offset counts from its first base whatever the start position.  Kept as written
 *   pruning      E:57-96: the heap starts with the creation's count, every group's end from the creator's group on pushes the
 *                edge's count inside that group (R:454-456 flushes every edge that exists, the reference's group too), the
 *                lowest leaves once capacity + 1 are held; edge_pruning_multiplicity is the lowest left
 * Inputs as phmm_assembly_kmers takes them, and
 *   read_sample [n_reads] or NULL (one sample)   any values; reads with equal values inside a region are one sample
 *   num_pruning_samples   1 .. PHMM_GRAPH_MAX_PRUNING_SAMPLES (the reference's default is 1)
 * Outputs.  A graph is a (k, region) pair in k-major order, o = k index * n_regions + region, n_graphs = n_k * n_regions:
 *   flags [n_graphs]   PHMM_ASM_REF_SHORT / _REF_NON_UNIQUE / _LOW_COMPLEXITY as phmm_assembly_kmers reports them.  A REF_SHORT
 *                graph is empty; the other two are still built
 *   n_vertices, n_edges, n_ref_path [n_graphs];  vertex_off, edge_off, ref_path_off [n_graphs+1]
 *   per vertex, in NodeIndex order, at vertex_off[o] + index:  vertex_seq  0 = the reference, 1 + r = read r of the region;
 *                vertex_pos  the creating occurrence, counted in the sequence (the read's window): the vertex's bytes are that
 *                sequence's [pos, pos + k), its suffix the last of them;  vertex_flags  PHMM_GRAPH_VERTEX_TRACKED = it is in
 *                kmer_to_vertex_map (what R:473-476 marks with "+"), PHMM_GRAPH_VERTEX_REF_SOURCE = the reference's first vertex
 *   per edge, in EdgeIndex order, at edge_off[o] + index:  edge_src, edge_dst (vertex indices inside the graph), edge_is_ref
 *                (bytes), edge_multiplicity, edge_pruning_multiplicity
 *   ref_path     reference_path as written (R:525-548): the vertex of every reference position 0 ..= len - k; empty for a
 *                reference of exactly k bases, where R:492 returns first, and for REF_SHORT
 *   ref_vertex [n_k x region_ref_off[n_regions]], read_vertex [n_k x read_off[n_reads]]   both NULL (not written) or k-major
 *                planes over ref_bases / read_bases as given: the vertex index a visited position lands on, UINT32_MAX
 *                elsewhere.  A later stage walks reads through the graph with these and needs no bytes
 * capacity [3] / required [3] count vertices, edges and ref_path entries, as phmm_assembly_regions does: when a capacity is too
 * small the call returns PHMM_ERR_EVENT_CAPACITY with `required` filled and nothing else written; all capacities 0 is the
 * way to ask, and the per-vertex, per-edge and ref_path arrays may then be NULL.
 * Limits: phmm_assembly_kmers' for bases and positions; PHMM_GRAPH_MAX_SAMPLES distinct read_sample values per region.  Device
 * workspace kept by the handle on top of phmm_assembly_kmers': 193 bytes per base and k (handles and edge slots per
 * position, the trie and edge tables, stamps and in-edges per vertex slot) and 28 per read and k; behind the sizes, 4 bytes
 * per edge and (1 + the region's samples), and the outputs.
 * The result is the same from run to run and whatever else is in the batch: which position claims a slot of a table is a
 * race that no output shows; the other atomics are minima and integer sums.
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offender): every case of phmm_assembly_kmers (with
 * ref_vertex / read_vertex for its id planes); num_pruning_samples outside its range; more than PHMM_GRAPH_MAX_SAMPLES samples
 * in a region; one vertex plane without the other; capacity or required NULL; a capacity above 0 whose arrays are NULL.
 * n_regions == 0 (required = {0, 0, 0}, the offset arrays hold their 0), regions without reads and empty reads are fine.  One
 * thread per handle.  Switch "asm_fingerprint_bits" (tests) cuts the trie table's fingerprints too.
 */
#define PHMM_GRAPH_MAX_SAMPLES 64u
#define PHMM_GRAPH_MAX_PRUNING_SAMPLES 8u
#define PHMM_GRAPH_VERTEX_TRACKED 1u
#define PHMM_GRAPH_VERTEX_REF_SOURCE 2u
int phmm_assembly_graph(phmm_handle *h, uint32_t n_regions, const uint32_t *region_ref_off, const uint8_t *ref_bases,
                        const uint32_t *region_read_off, const uint32_t *read_off, const uint8_t *read_bases,
                        const uint8_t *read_quals, const uint32_t *read_first, const uint32_t *read_len,
                        const uint32_t *read_sample, uint32_t n_k, const uint32_t *k, uint32_t min_base_quality,
                        uint32_t num_pruning_samples, const uint32_t *capacity, uint32_t *required, uint32_t *flags,
                        uint32_t *n_vertices, uint32_t *n_edges, uint32_t *n_ref_path, uint32_t *vertex_off, uint32_t *edge_off,
                        uint32_t *ref_path_off, uint32_t *vertex_seq, uint32_t *vertex_pos, uint8_t *vertex_flags,
                        uint32_t *edge_src, uint32_t *edge_dst, uint8_t *edge_is_ref, uint32_t *edge_multiplicity,
                        uint32_t *edge_pruning_multiplicity, uint32_t *ref_path, uint32_t *ref_vertex, uint32_t *read_vertex);

/*
 * phmm_assembly_prune -- what create_graph does to the raw graph before it looks for paths (A:1041-1073, A:1118-1136), for many
 * graphs in ONE call: prune_low_weight_chains with the production pruner (the low-weight one; the adaptive pruner is LEFT OUT),
 * the orphans, the cycle verdict, the reference ends, the vertices dangling-end recovery starts from, and
 * remove_paths_not_connected_to_ref.  Integers and bytes: every output EQUALS the reference's.  A, R as above,
 * C = src/graphs/chain_pruner.rs, L = src/graphs/low_weight_chain_pruner.rs, B = src/graphs/base_graph.rs.  Degrees count
 * edges.  Three graphs: G0 = the input without its absent elements; G1 = G0 after CHAINS if asked, else G0; G2 = G1 after
 * CONNECT if asked, else G1.
 *   CHAINS       (C:39-56) a vertex is interior if its in-degree and its out-degree are 1.  An edge's chain head is the edge
 *                itself if its source is not interior, else the head of the source's one in-edge; an edge on a ring of interior
 *                vertices has none.  find_all_chains (C:58-80) finds a head exactly when its source can be reached in G0 from
 *                a vertex of in-degree 0; a component without such a vertex yields no chain and loses nothing.  A found chain
 *                is removed if every edge of it has pruning multiplicity < prune_factor and is not is_ref (L:24-36): nothing
 *                with factor 0.  Then every vertex without an edge is removed unless G0 has exactly one vertex (B:392-406:
 *                the orphans are listed before any is removed, and is_ref_source of an isolated vertex asks for a node count
 *                of 1)
 *   on G1        PHMM_PRUNE_HAS_CYCLE: a directed cycle, a self-loop included (B:615-617).  ref_source / ref_sink: the lowest
 *                vertex index for which is_ref_source / is_ref_sink holds (B:339-387, B:411-428), its "the graph has one node"
 *                evaluated on G1; UINT32_MAX if there is none, and PHMM_PRUNE_NO_REF_ENDS if either is missing.  Per vertex
 *                PHMM_PRUNE_DANGLING_TAIL: out-degree 0 and not is_ref_sink (R:792-797); PHMM_PRUNE_DANGLING_HEAD: in-degree 0
 *                and not is_ref_source (R:837-842)
 *   CONNECT      (B:626-656) every vertex of G1 goes, with its edges, unless it can be reached forwards from ref_source AND
 *                backwards from ref_sink.  A graph with NO_REF_ENDS stays G1 (the reference panics there)
 * The LOW_COMPLEXITY verdict of A:1066 is the flag phmm_assembly_graph already reports: pruning changes neither
 * non_unique_kmers nor kmer_to_vertex_map, so it is not computed again here.
 * Inputs: the arrays as phmm_assembly_graph writes them,
 *   vertex_off, edge_off [n_graphs+1]; edge_src, edge_dst (indices inside the graph), edge_is_ref, edge_pruning_multiplicity
 *   vertex_absent, edge_absent   both NULL or both given: a nonzero byte marks an element that is not in the graph (a vacant
 *                slot of a StableGraph), so that a second call can run on a graph the caller has changed -- CONNECT comes
 *                behind dangling-end recovery
 *   ops          PHMM_PRUNE_OP_CHAINS | PHMM_PRUNE_OP_CONNECT
 *   prune_factor [n_graphs]   the coverage correction of A:245-255 is the caller's arithmetic
 * Outputs:
 *   graph_flags, n_chains (found), n_chains_removed, n_vertices_left, n_edges_left (of G2), ref_source, ref_sink [n_graphs]
 *   edge_chain [edges]   the head's EdgeIndex; UINT32_MAX for an edge in no found chain, and everywhere without CHAINS
 *   edge_state [edges], vertex_state [vertices]   PHMM_PRUNE_ABSENT (as given), _REMOVED_CHAINS, _REMOVED_CONNECT; on vertices
 *                the two dangling bits too (of G1, whatever CONNECT removes)
 * Device workspace kept by the handle: 20 bytes per vertex and 5 per edge, beside the staged arrays.  One workgroup works on a
 * graph, so a call with one huge graph runs on one compute unit.  The result is the same from run to run: the atomics are
 * integer sums, ORs and minima, and a mark is only ever set.
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offender): ops 0 or with unknown bits; one mask without
 * the other; a NULL array that has elements; offsets that do not start at 0 or decrease; an endpoint >= the graph's
 * n_vertices; a present edge with an absent endpoint.  n_graphs == 0, graphs without vertices and graphs without edges are
 * fine.  One thread per handle.
 */
#define PHMM_PRUNE_OP_CHAINS 1u
#define PHMM_PRUNE_OP_CONNECT 2u
#define PHMM_PRUNE_HAS_CYCLE 1u
#define PHMM_PRUNE_NO_REF_ENDS 2u
#define PHMM_PRUNE_ABSENT 1u
#define PHMM_PRUNE_REMOVED_CHAINS 2u
#define PHMM_PRUNE_REMOVED_CONNECT 4u
#define PHMM_PRUNE_DANGLING_TAIL 8u
#define PHMM_PRUNE_DANGLING_HEAD 16u
int phmm_assembly_prune(phmm_handle *h, uint32_t n_graphs, const uint32_t *vertex_off, const uint32_t *edge_off,
                        const uint32_t *edge_src, const uint32_t *edge_dst, const uint8_t *edge_is_ref,
                        const uint32_t *edge_pruning_multiplicity, const uint8_t *vertex_absent, const uint8_t *edge_absent,
                        uint32_t ops, const uint32_t *prune_factor, uint32_t *graph_flags, uint32_t *n_chains,
                        uint32_t *n_chains_removed, uint32_t *n_vertices_left, uint32_t *n_edges_left, uint32_t *ref_source,
                        uint32_t *ref_sink, uint32_t *edge_chain, uint8_t *edge_state, uint8_t *vertex_state);

/*
 * phmm_assembly_recover -- dangling-end recovery, what get_assembly_result does next (A:1118-1131): recover_dangling_tails, then
 * recover_dangling_heads on the graph the tails left, for many graphs in ONE call.  Integers and bytes: every output EQUALS the
 * reference's.  R = src/read_threading/read_threading_graph.rs:779-1766, B = src/graphs/base_graph.rs,
 * T = src/read_threading/abstract_read_threading_graph.rs:91-125, 202-212, E = src/graphs/multi_sample_edge.rs.
 * Modes: recover_all_dangling_branches = false (the default: give_up_at_branch = true in both find_path_* functions).
 * recover_all = true is LEFT OUT; the config has no field for it.  Both head merges are in: min_matching_bases < 0 (the command
 * line's default is -1) takes merge_dangling_head_legacy with best_prefix_match_legacy and get_max_mismatches_legacy, >= 0 takes
 * merge_dangling_head with best_prefix_match; the tail's matching_suffix test (R:987-993) reads the same value.  As written:
 *   order        all tails are listed in NodeIndex order before any is touched (R:792-797) and taken in that order, then the
 *                heads likewise on the graph the tails left.  A merge changes degrees that a later end reads, so the ends of a
 *                graph are taken strictly one after the other
 *   find_path    R:1651-1692 in full: the low-weight reset against prune_factor, the loop check, done / return_path of
 *                R:1505-1524 and R:1595-1614; then the is_ref_source / is_ref_sink / length refusals (R:1386-1390 with
 *                max(1, min_dangling_branch_length) for a tail, R:1453-1457 with the length as given for a head)
 *   reference path   downwards get_next_reference_vertex(v, true, the in-edge of alt_path[1]), upwards
 *                get_prev_reference_vertex; edges_directed lists the NEWEST edge first, which decides among several reference
 *                out-edges or reference-node predecessors.  An edge this call adds is newer than every edge of the input
 *   strings      the suffix byte per vertex; for a head a vertex of in-degree 0 gives its whole k-mer reversed (R:1741-1750)
 *   alignment    reference-path string against alt-path string, phmm_sw_align's aligner restated for LeadingInDel, then
 *                remove_trailing_deletions; cigar_is_okay_to_merge with MAX_CIGAR_COMPLEXITY = 3
 *   merges       merge_dangling_tail (longest_suffix_match capped by the last element, the leading-deletion correction,
 *                ref_index_to_merge <= 0 refused), the two head merges, extend_dangling_path_against_reference (R:1209-1291: the
 *                dangling source's out-edge goes, num_nodes_to_extend vertices with the bytes sequence_to_extend[i..i+k] are
 *                chained by edges of the removed edge's multiplicity).  A new edge is MultiSampleEdge::new(false, multiplicity,
 *                num_pruning_samples): its heap holds the one count, so its pruning multiplicity IS its multiplicity (E:119-131)
 * The reuse of vacant petgraph slots by the caller's own add_edge is NOT modelled: new elements are reported in creation order,
 * which is what a caller with a StableGraph needs (the newest edge comes first in edges_directed).
 * cfg points to a phmm_recover_config (declared `const void *` like phmm_finalize_reads' cfg):
 *   ops          PHMM_RECOVER_OP_TAILS | PHMM_RECOVER_OP_HEADS
 *   min_dangling_branch_length, min_matching_bases, max_mismatches_in_dangling_head (the defaults: 4, -1, -1)
 *   num_pruning_samples   1 .. PHMM_GRAPH_MAX_PRUNING_SAMPLES (the capacity of a new edge's heap: no output depends on it)
 *   sw_parameters         the dangling-end Smith-Waterman parameters (STANDARD_NGS = 25, -50, -110, -6)
 * Inputs: the region arrays as phmm_assembly_graph takes them (a vertex's bytes are vertex_seq / vertex_pos into them), n_k, k
 * and the k-major graph layout (n_graphs = n_k * n_regions); the graph arrays as phmm_assembly_graph writes them: vertex_off,
 * edge_off, vertex_seq, vertex_pos, edge_src, edge_dst, edge_is_ref, edge_multiplicity, edge_pruning_multiplicity;
 *   vertex_absent, edge_absent   both NULL or both given, nonzero = not in the graph (phmm_assembly_prune's states)
 *   graph_flags [n_graphs] or NULL   phmm_assembly_prune's: a graph with PHMM_PRUNE_HAS_CYCLE is refused (the caller drops it
 *                before this stage).  Cycles are not looked for again: every walk ends after vertices + 1 steps
 *   prune_factor [n_graphs]
 * Outputs.  capacity [3] / required [3] count ends, new edges and new vertices, as phmm_assembly_graph's do: when a capacity is
 * too small the call returns PHMM_ERR_EVENT_CAPACITY with `required` filled and nothing else written; all capacities 0 is the
 * way to ask (the call does all its work either way: the sizes are known only once the ends have been taken).
 *   per graph    n_tails, n_tails_recovered, n_heads, n_heads_recovered, n_new_edges, n_new_vertices, n_rounds [n_graphs];
 *                end_off, new_edge_off, new_vertex_off [n_graphs+1].  n_rounds: the rounds a speculate-and-commit schedule
 *                would need -- all pending ends of a kind resolved at once, committed in order up to the first end that inspected
 *                a vertex whose edges an end of the same round changed; 1 per kind with ends where ends do not interfere
 *   per end, in processing order   end_vertex; end_kind (PHMM_RECOVER_KIND_*); end_status (PHMM_RECOVER_END_*, one per exit of
 *                the reference); end_alt_len, end_ref_len: the two strings' lengths (0 where none was aligned); end_n_cigar and
 *                end_cigar [ends x 4]: the first 4 elements in BAM encoding, the trailing deletion removed; end_edge: the new
 *                edge it made, counted inside the graph's new edges, or UINT32_MAX
 *   per new edge, in creation order   new_edge_src, new_edge_dst (new vertices are numbered n_vertices + i inside the graph;
 *                both UINT32_MAX for a new edge that a later extension took out again), new_edge_multiplicity,
 *                new_edge_pruning_multiplicity; is_ref is 0 by construction
 *   per new vertex   new_vertex_kmer [new vertices x max(k)]: its k bytes, zeros behind them.  They are no occurrence in any
 *                input sequence
 *   edge_removed [edges]   1 for the out-edge that an extension took out
 * PHMM_RECOVER_END_NO_MERGE_POINT: best_prefix_match_legacy met no mismatch inside the first element, or best_prefix_match ran
 * to an index <= 0 (R:1179-1181).  PHMM_RECOVER_END_REFERENCE_FAILS: the reference itself panics or never returns here (a merge
 * index past the reference path at R:1031 with min_matching_bases = 0, a walk through a cycle); nothing is merged.
 * Deviation from a batch-parallel schedule: one workgroup (one wave) works on a graph and takes its ends one after the other
 * with an aligner of its own -- an anti-diagonal sweep, not phmm_sw_align's kernels.  A call with one huge graph runs on one
 * compute unit.  Limits: 30 000 vertices per graph (a backtrack entry has 16 bits); max |weight| x (2 x (vertices + max k + 2)
 * + 2) below 1e9.  Device workspace kept by the handle: 41 bytes per vertex slot and 17 per edge slot -- a graph's slots are its
 * own plus (k + 1) edges and k vertices per candidate head and one edge per candidate tail -- and per workgroup in flight a slab
 * of 2 (L + 1)^2 + 46 L bytes, L = the most vertices of a graph with ends + max k + 2 -- the bound of a path, not the lengths
 * the ends turn out to have; as many workgroups run as 512 MiB of slabs allow, and at least one: a slab larger than that is
 * allocated at its size (1.8 GB at the vertex limit), and the handle keeps half as much again.
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offender): the cases of phmm_assembly_prune for
 * offsets, endpoints and masks; region offsets that do not start at 0 or decrease, a read window outside its read; vertex_seq /
 * vertex_pos outside their sequence; k outside 1 .. PHMM_ASM_MAX_K; ops 0 or with unknown bits; num_pruning_samples out of
 * range; cfg, capacity or required NULL; a graph flagged cyclic; a graph above the limits; a capacity above 0 whose arrays are
 * NULL.  n_graphs == 0, graphs without vertices and graphs without dangling ends are fine.  One thread per handle.
 */
#define PHMM_RECOVER_OP_TAILS 1u
#define PHMM_RECOVER_OP_HEADS 2u
#define PHMM_RECOVER_KIND_TAIL 0u
#define PHMM_RECOVER_KIND_HEAD 1u
#define PHMM_RECOVER_END_NO_PATH 0u
#define PHMM_RECOVER_END_LOOP 1u
#define PHMM_RECOVER_END_AT_REF_END 2u
#define PHMM_RECOVER_END_TOO_SHORT 3u
#define PHMM_RECOVER_END_CIGAR_NOT_OKAY 4u
#define PHMM_RECOVER_END_TOO_FEW_MATCHING 5u
#define PHMM_RECOVER_END_WHOLE_INSERTION 6u
#define PHMM_RECOVER_END_TOO_MANY_MISMATCHES 7u
#define PHMM_RECOVER_END_CANNOT_PUSH_REF 8u
#define PHMM_RECOVER_END_CANNOT_EXTEND 9u
#define PHMM_RECOVER_END_MERGED 10u
#define PHMM_RECOVER_END_NO_MERGE_POINT 11u
#define PHMM_RECOVER_END_REFERENCE_FAILS 12u
typedef struct phmm_recover_config {
    uint32_t ops;
    int32_t min_dangling_branch_length;
    int32_t min_matching_bases;
    int32_t max_mismatches_in_dangling_head;
    uint32_t num_pruning_samples;
    phmm_sw_parameters sw_parameters;
} phmm_recover_config;
int phmm_assembly_recover(phmm_handle *h, const void *cfg, uint32_t n_regions, const uint32_t *region_ref_off,
                          const uint8_t *ref_bases, const uint32_t *region_read_off, const uint32_t *read_off,
                          const uint8_t *read_bases, const uint32_t *read_first, const uint32_t *read_len, uint32_t n_k,
                          const uint32_t *k, const uint32_t *vertex_off, const uint32_t *edge_off, const uint32_t *vertex_seq,
                          const uint32_t *vertex_pos, const uint32_t *edge_src, const uint32_t *edge_dst,
                          const uint8_t *edge_is_ref, const uint32_t *edge_multiplicity,
                          const uint32_t *edge_pruning_multiplicity, const uint8_t *vertex_absent, const uint8_t *edge_absent,
                          const uint32_t *graph_flags, const uint32_t *prune_factor, const uint32_t *capacity, uint32_t *required,
                          uint32_t *n_tails, uint32_t *n_tails_recovered, uint32_t *n_heads, uint32_t *n_heads_recovered,
                          uint32_t *n_new_edges, uint32_t *n_new_vertices, uint32_t *n_rounds, uint32_t *end_off,
                          uint32_t *new_edge_off, uint32_t *new_vertex_off, uint32_t *end_vertex, uint32_t *end_kind,
                          uint32_t *end_status, uint32_t *end_alt_len, uint32_t *end_ref_len, uint32_t *end_n_cigar,
                          uint32_t *end_cigar, uint32_t *end_edge, uint32_t *new_edge_src, uint32_t *new_edge_dst,
                          uint32_t *new_edge_multiplicity, uint32_t *new_edge_pruning_multiplicity, uint8_t *new_vertex_kmer,
                          uint8_t *edge_removed);

/*
 * phmm_assembly_seqgraph -- the zipped sequence graph, what get_assembly_result does behind the pruned graph (A:1154-1259):
 * to_sequence_graph (B:54-84), clean_non_ref_paths (B:716-768), the first zip_linear_chains (S:189-369, called at A:1251),
 * remove_singleton_orphan_vertices (B:392-406) and remove_vertices_not_connected_to_ref_regardless_of_edge_direction
 * (B:774-793 with B:686-709), for many graphs in ONE call.  It stops at the graph the reference would print as "1.2.pruned",
 * in front of simplify_graph (A:1284); simplify_graph and the path finder are LEFT OUT.  Integers and bytes: every output
 * EQUALS a serial restatement of the reference.  A, B as above, S = src/graphs/seq_graph.rs.  Degrees count edges.
 * Numbering: petgraph's reuse of vacant slots is NOT modelled.  A new vertex or edge takes a fresh index behind all existing
 * ones; the output is the present elements in ascending model index, renumbered compactly.  So unmerged vertices keep their
 * relative order and merged vertices follow in the order of their zip starts; untouched edges keep their relative order and
 * re-created edges follow in creation order.  (The reference's own tests compare sequence graphs by content: graph_equals.)
 *   (1) conversion   sequence vertex i is the i-th present vertex, sequence edge j the j-th present edge.  A vertex with
 *                in-degree 0 among the present edges carries all its k bytes, any other its last byte.  An edge keeps is_ref
 *                and multiplicity
 *   (2) clean    nothing unless both reference ends exist (the lowest index for which is_ref_source / is_ref_sink holds, with
 *                "the graph has one node" as written).  The removed in-edges are the least fixed point of: a non-reference
 *                edge goes if its target is the reference source or the source of a removed edge; the out-edge side is the
 *                mirror from the reference sink, on the graph the first half left.  Then the orphans go (B:766).  The
 *                reference pops an edge it has removed, and panics, where a vertex's edge list is pushed a second time and
 *                still holds a non-reference edge; whether it still does depends on the heap's order.  The contract is the
 *                order-free superset: a vertex that is pushed twice (it is the swept end, or the far end of a removed edge,
 *                two times in all) and whose list held a non-reference edge gives the graph PHMM_SEQ_REFERENCE_FAILS and empty
 *                outputs.  ("The sink is gone after the first half" cannot happen: only non-reference edges go there.)
 *                Behind PHMM_PRUNE_OP_CONNECT on an acyclic graph this step removes nothing
 *   (3) zip      a vertex is a start if its out-degree is 1 and its in-degree is not 1, or its one predecessor has out-degree
 *                above 1; starts are listed in ascending index before anything changes.  A chain runs from its start while
 *                the last vertex has out-degree 1, the target in-degree 1, the target is not the last vertex and both have
 *                the same is_reference_node.  A chain of two or more vertices becomes one vertex with the chain's bytes; it
 *                gets copies of the last vertex's out-edges, newest first, then of the first vertex's in-edges, newest first,
 *                as that list stands then.  As written: the vertex behind a reference / non-reference break is no start and
 *                stays unzipped with what follows it; last -> first gives a self-loop; an edge from the end of one chain to
 *                the start of another is copied twice and survives once, created at the later merge; a ring of interior
 *                vertices has no start and stays
 *   (4) orphans  listed before any goes; an isolated vertex stays only if it is the graph's one vertex
 *   (5) connectivity   kept: the reference source, what reaches it backwards and what it reaches forwards -- NOT weak
 *                connectivity.  Without a reference source every vertex goes
 * Inputs: the region arrays, n_k, k and the k-major graph layout as phmm_assembly_recover takes them; vertex_off, edge_off,
 * edge_src, edge_dst, edge_is_ref, edge_multiplicity of the graphs as they stand (recovery's elements behind each graph's own);
 *   vertex_seq, vertex_pos   of the raw vertices only: graph g's rows start at vertex_off[g] - new_vertex_off[g]
 *   new_vertex_off [n_graphs+1], new_vertex_kmer [new vertices x max(k)]   both NULL or both given, as phmm_assembly_recover
 *                writes them: the last new_vertex_off[g+1] - new_vertex_off[g] vertices of graph g take their k bytes from the rows
 *   vertex_absent, edge_absent   both NULL or both given, nonzero = not in the graph
 *   graph_flags [n_graphs] or NULL   phmm_assembly_prune's: a graph with PHMM_PRUNE_HAS_CYCLE or PHMM_PRUNE_NO_REF_ENDS is the
 *                caller's to drop; it gets PHMM_SEQ_SKIPPED and empty outputs
 * The regions' bases are staged again (the device needs one byte per vertex and k per source vertex, and the chain hands them
 * over in no smaller form without host work between the calls).
 * Outputs.  capacity [3] / required [3] count sequence vertices, sequence edges and sequence bytes, as phmm_assembly_graph's
 * do: when a capacity is too small the call returns PHMM_ERR_EVENT_CAPACITY with `required` filled and nothing else written;
 * all capacities 0 is the way to ask (the call does all its work either way, and only the sizes come back).
 *   per graph    seq_status (PHMM_SEQ_*), n_seq_vertices, n_seq_edges, n_seq_bases, n_chains_zipped (chains merged),
 *                n_removed_clean (edges step 2 removed), n_removed_unconnected (vertices step 5 removed), seq_ref_source,
 *                seq_ref_sink (of the final graph, UINT32_MAX if none) [n_graphs]; seq_vertex_off, seq_edge_off, seq_base_off
 *                [n_graphs+1]
 *   per sequence vertex   seq_vertex_base_off (inside the graph's bytes; a vertex's bytes end where the next one's start);
 *                seq_vertex_first: the input vertex that is the chain's first, or the vertex itself; seq_vertex_n_merged
 *   per sequence edge   seq_edge_src, seq_edge_dst (indices inside the graph), seq_edge_is_ref, seq_edge_multiplicity
 *   seq_bases [bytes]; vertex_to_seq [vertices] or NULL: the sequence vertex that holds the input vertex's bytes, UINT32_MAX
 *                where it is gone
 * One workgroup of 256 lanes works on a graph, in the device workspace whatever the graph's size (no LDS copy of small
 * graphs); a second kernel sums the sizes and a third writes the output at each graph's offsets, so only the zipped graphs
 * (and vertex_to_seq, if asked for) cross to the host.  Device workspace kept by the handle: 84 bytes per vertex, 5 per edge
 * and 16 per sort slot (a graph's edge count rounded up to a power of two).  Limits: a graph's vertices below 2^31 - 1;
 * vertices x max(k) within 32 bits.  The result is the same from run to run and whatever else is in the batch: the atomics
 * are integer sums, ORs, minima and maxima, and the one atomic append feeds a sort of distinct keys.
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offender): the cases of phmm_assembly_prune and
 * phmm_assembly_recover for offsets, endpoints, masks, region offsets, read windows, vertex_seq / vertex_pos and k; one of
 * new_vertex_off / new_vertex_kmer without the other; capacity or required NULL; a NULL array that has elements; a capacity
 * above 0 whose arrays are NULL; a graph above the limits.  n_graphs == 0, empty graphs and graphs without edges are fine.
 * One thread per handle.
 */
#define PHMM_SEQ_OK 0u
#define PHMM_SEQ_SKIPPED 1u
#define PHMM_SEQ_REFERENCE_FAILS 2u
int phmm_assembly_seqgraph(phmm_handle *h, uint32_t n_regions, const uint32_t *region_ref_off, const uint8_t *ref_bases,
                           const uint32_t *region_read_off, const uint32_t *read_off, const uint8_t *read_bases,
                           const uint32_t *read_first, const uint32_t *read_len, uint32_t n_k, const uint32_t *k,
                           const uint32_t *vertex_off, const uint32_t *edge_off, const uint32_t *vertex_seq,
                           const uint32_t *vertex_pos, const uint32_t *edge_src, const uint32_t *edge_dst,
                           const uint8_t *edge_is_ref, const uint32_t *edge_multiplicity, const uint32_t *new_vertex_off,
                           const uint8_t *new_vertex_kmer, const uint8_t *vertex_absent, const uint8_t *edge_absent,
                           const uint32_t *graph_flags, const uint32_t *capacity, uint32_t *required, uint32_t *seq_status,
                           uint32_t *n_seq_vertices, uint32_t *n_seq_edges, uint32_t *n_seq_bases, uint32_t *n_chains_zipped,
                           uint32_t *n_removed_clean, uint32_t *n_removed_unconnected, uint32_t *seq_ref_source,
                           uint32_t *seq_ref_sink, uint32_t *seq_vertex_off, uint32_t *seq_edge_off, uint32_t *seq_base_off,
                           uint32_t *seq_vertex_base_off, uint32_t *seq_vertex_first, uint32_t *seq_vertex_n_merged,
                           uint32_t *seq_edge_src, uint32_t *seq_edge_dst, uint8_t *seq_edge_is_ref,
                           uint32_t *seq_edge_multiplicity, uint8_t *seq_bases, uint32_t *vertex_to_seq);

/*
 * phmm_assembly_best_paths -- the k best haplotype paths of many sequence graphs in ONE call: what find_best_path
 * (A:709-899) asks of GraphBasedKBestHaplotypeFinder, and Path::get_bases behind it.  F = src/graphs/k_best_haplotype_finder.rs,
 * G = src/graphs/graph_based_k_best_haplotype_finder.rs, K = src/graphs/k_best_haplotype.rs, P = src/graphs/path.rs.  Taken as
 * written, not repaired; every output EQUALS a serial restatement of the reference, scores to the bit.  simplify_graph, the
 * one-vertex "dummy" fix-up (A:1319-1331) and the CIGAR filters (A:795-858) are LEFT OUT.
 * The graph is taken as created: an edge's index inside its graph is its petgraph EdgeIndex, a vertex's out-edges iterate
 * newest first (descending index).  A vertex may have 0 bytes.
 *   (1) cycles   F:71-182, only if the WHOLE graph is cyclic (parts the source cannot reach included).  From every source a
 *                depth-first walk over out-edges, newest first, with a fresh visited set per source; the set is never
 *                shrunk on return, so an edge to ANY visited vertex goes -- cross and forward edges too.  A sink returns
 *                true at once: it is never marked and never explored, so edges into a sink stay and its out-edges are not
 *                walked.  Every child is visited.  A visited vertex that reaches no sink through first visits goes with
 *                its edges; unvisited vertices stay.  No path found: PHMM_PATHS_NO_PATH (first assert; also a cyclic graph
 *                with no source); nothing to remove: PHMM_PATHS_CYCLES_STAY (second assert: the cycle is out of reach).
 *                Both give empty outputs and zero marks
 *   (2) search   G:64-132.  The queue starts with a zero-edge path per source.  Pop the greatest.  At a sink it is a result
 *                and is not extended.  Elsewhere count[v] += 1 and, if count[v] < max_paths, one child per present out-edge
 *                is pushed.  Stops when the queue is empty or max_paths results exist
 *   (3) score    child = parent + (log10(m) - log10(T)), T the sum of the vertex's present out-edge multiplicities in 64
 *                bits: three roundings, no contraction.  Order (K:103-112): OrderedFloat's -- NaN greatest and equal to
 *                itself, -0.0 equal to 0.0 -- then the lexicographically smaller edge list wins, a proper prefix before its
 *                extension; zero-edge paths of several sources, which tie completely, go in ascending vertex index.  m == 0
 *                with T > 0 gives -inf; m == 0 with T == 0 gives NaN (the dummy edge's path, which pops first); a NaN is
 *                written as 0x7ff8000000000000 whatever sign the subtraction gave it.  is_ref: the AND of the edges'
 *                is_ref, true for a zero-edge path
 *   (4) log10    the handle keeps L[n] = log10((double)n) on the device, built on the host by the C library's log10, one
 *                call per entry, L[0] = -inf, grown on demand to the largest per-vertex total (over the out-edges as given)
 *                of a call, up to PHMM_PATHS_MAX_WEIGHT.  A graph with a larger total gets PHMM_PATHS_WEIGHT_RANGE
 *   (5) bases    P:234-267: the first vertex's bytes, then each edge target's
 *   (6) budget   a graph whose search would create more than max_nodes_per_graph tree nodes (the sources' included) gets
 *                PHMM_PATHS_BUDGET and no paths; the marks and counts of step 1 stay.  The pool of a graph is
 *                min(budget, sources + (max_paths - 1) x edges), which no search can exceed
 *   (7) duplicates   A:770 with Haplotype::eq on bytes, only with the region arrays: for region r the paths of graphs
 *                k x n_regions + r in k order and rank order are what find_best_path meets.  path_first_equal[p]:
 *                UINT32_MAX = first of its bytes; PHMM_PATHS_EQUALS_REF = the region's reference bytes (the result set
 *                starts with the reference haplotype); else the call-wide index of the earliest path with these bytes
 * Inputs: n_graphs; seq_vertex_off, seq_edge_off, seq_base_off [n_graphs+1], seq_vertex_base_off, seq_edge_src, seq_edge_dst,
 * seq_edge_is_ref, seq_edge_multiplicity, seq_bases as phmm_assembly_seqgraph writes them;
 *   seq_status [n_graphs] or NULL   a graph whose status is not PHMM_SEQ_OK gets PHMM_PATHS_SKIPPED
 *   graph_source, graph_sink [n_graphs]   seq_ref_source / seq_ref_sink; UINT32_MAX in either gives PHMM_PATHS_NO_ENDS (A:739-742)
 *   vertex_role [vertices] or NULL   bit 0 a source, bit 1 a sink; when given it replaces the two arrays (they may be NULL).
 *                An empty source or sink set gives an acyclic graph 0 paths
 *   max_paths    num_best_haplotypes_per_graph; UINT32_MAX = usize::MAX.  max_nodes_per_graph: nonzero
 *   n_regions, n_k, region_ref_off [n_regions+1], ref_bases   all given (n_graphs == n_k x n_regions, k-major) or 0 / NULL
 * Outputs.  capacity [3] / required [3] count paths, path edges and haplotype bytes, as phmm_assembly_seqgraph's do:
 * PHMM_ERR_EVENT_CAPACITY with `required` filled and nothing else written; all capacities 0 asks for the sizes.
 *   per graph    paths_status (PHMM_PATHS_*), n_paths, n_popped (queue pops), n_cycle_edges_removed (edges gone behind step 1,
 *                those of removed vertices included), n_cycle_vertices_removed [n_graphs]; path_off, path_edge_off,
 *                hap_base_off [n_graphs+1]
 *   per path, call-wide, a graph's paths in pop order   path_score, path_is_ref, path_n_edges [paths]; hap_off [capacity[0]+1]:
 *                path p's bytes are hap_bases[hap_off[p] .. hap_off[p+1]) -- the alt_off / alt_bases of phmm_calculate_cigar;
 *                path_first_equal [paths] or NULL
 *   path_edges [path edges]   indices inside the graph, a path's edges in order, the paths one behind the other
 *   hap_bases [bytes]; edge_removed [edges], vertex_removed [vertices] or NULL: nonzero = gone in step 1 (an edge: bit 0 the
 *                walk removed it, bit 1 it went with a vertex)
 * One wave works on a graph, in the handle's device workspace (20 bytes per vertex, 4 per edge, 45 per node of the pools);
 * the queue is an unsorted array and a pop is a wave argmax under the reference's order, ties by walking the two paths to
 * their common ancestor in the search tree.  Then an offsets kernel, an output kernel (a wave per path) and the duplicate
 * kernel (a wave per path).  One writer per element; the bytes of a call are the same from run to run and whatever else is
 * in the batch.
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offender): offsets not starting at 0 or
 * descending; an endpoint outside its graph; a seq_vertex_base_off past the graph's bytes or descending; a source or sink
 * that is neither a vertex nor UINT32_MAX; a role above 3; max_paths or max_nodes_per_graph 0; the region arguments given
 * in part, or n_k x n_regions != n_graphs; path_first_equal without them; capacity or required NULL; a NULL array that has
 * elements; a capacity above 0 whose arrays are NULL; node pools beyond 32 bits in sum; paths, path edges or haplotype
 * bytes that reach 2^32 - 1 in sum (known only behind the search: no capacity could hold them, so it is not
 * PHMM_ERR_EVENT_CAPACITY).  n_graphs == 0, empty graphs and
 * graphs without edges are fine.  One thread per handle.
 */
#define PHMM_PATHS_OK 0u
#define PHMM_PATHS_SKIPPED 1u
#define PHMM_PATHS_NO_ENDS 2u
#define PHMM_PATHS_NO_PATH 3u
#define PHMM_PATHS_CYCLES_STAY 4u
#define PHMM_PATHS_WEIGHT_RANGE 5u
#define PHMM_PATHS_BUDGET 6u
#define PHMM_PATHS_MAX_WEIGHT 1048576u
#define PHMM_PATHS_EQUALS_REF 4294967294u
int phmm_assembly_best_paths(phmm_handle *h, uint32_t n_graphs, const uint32_t *seq_vertex_off, const uint32_t *seq_edge_off,
                             const uint32_t *seq_base_off, const uint32_t *seq_vertex_base_off, const uint32_t *seq_edge_src,
                             const uint32_t *seq_edge_dst, const uint8_t *seq_edge_is_ref, const uint32_t *seq_edge_multiplicity,
                             const uint8_t *seq_bases, const uint32_t *seq_status, const uint32_t *graph_source,
                             const uint32_t *graph_sink, const uint8_t *vertex_role, uint32_t max_paths,
                             uint32_t max_nodes_per_graph, uint32_t n_regions, uint32_t n_k, const uint32_t *region_ref_off,
                             const uint8_t *ref_bases, const uint32_t *capacity, uint32_t *required, uint32_t *paths_status,
                             uint32_t *n_paths, uint32_t *n_popped, uint32_t *n_cycle_edges_removed,
                             uint32_t *n_cycle_vertices_removed, uint32_t *path_off, uint32_t *path_edge_off,
                             uint32_t *hap_base_off, double *path_score, uint8_t *path_is_ref, uint32_t *path_n_edges,
                             uint32_t *hap_off, uint32_t *path_first_equal, uint32_t *path_edges, uint8_t *hap_bases,
                             uint8_t *edge_removed, uint8_t *vertex_removed);

/*
 * phmm_trim_regions -- what the reference's call_region (src/haplotype/haplotype_caller_engine.rs:1194-1243) does with the
 * assembler's haplotypes before a likelihood is computed, for many regions in ONE call: get_variation_events, the trimmer's
 * two spans, every haplotype cut to the padded span, duplicates folded, the rest in the reference's order.  Integers and
 * bytes: every output EQUALS the reference's.  T = src/assembly/assembly_region_trimmer.rs, H = src/haplotype/haplotype.rs,
 * U = src/reads/alignment_utils.rs, S = src/assembly/assembly_result_set.rs, I = src/utils/simple_interval.rs.  Per region:
 *   event maps   build_event_maps_for_haplotypes as phmm_discover_events step 1 restates it (the same kernel).  A haplotype
 *                whose map fails gives the region its PHMM_EV_STATUS_* (the first such haplotype's): call_region returns the
 *                empty model there (:1197-1204).  Every other output of that region is 0 / PHMM_TRIM_FATE_NOT_TRIMMED
 *   spans        AssemblyRegionTrimmer::trim (T:61-131) with legacy_trimming = false, as call_region passes it.  Only events
 *                whose span overlaps the active span count (I:201-205 through :341-343; the three clauses of I:245-249 say the
 *                same of well-formed intervals); with none the region has no variation: variation_present 0, no output
 *                haplotypes, spans 0.  variant span = [min start, max end] & active span; per event the padding is
 *                padding[1] if its CACHED type is INDEL (a SNP joined with an insertion stays a SNP), else padding[0];
 *                min(start.saturating_sub(padding)), max(end + padding), & the region's padded span.  The BTreeSet's order and
 *                dedupe (src/model/variant_context.rs:69-82) change neither extreme: the device reduces over all haplotype events
 *   STR padding  get_num_tandem_repeat_units (src/model/variant_context_utils.rs:32-79) returns Some only with NO alternate
 *                allele (:74); an event of an event map has exactly one, so the arm that adds padding[2] (T:103-108) has no
 *                input and no repeat scan runs.  Kept as written; tests/test_region_trim_oracle.py runs the function itself.
 *                What the arm does do for every indel is slice the reference bases from start + 1 - padded span start
 *                (src/annotator/tandem_repeat.rs:21-25): an indel that starts more than one base in front of the region's
 *                padded span, or whose index lies behind the region's reference bases, panics there:
 *                PHMM_TRIM_STATUS_REPEAT_SLICE, every other output of the region 0 / NOT_TRIMMED
 *   new spans    trim_with_padded_span (src/assembly/assembly_region.rs:323-339): active & variant span, padded & padded
 *                variant span.  They feed phmm_finalize_reads with PHMM_FIN_REGION as they are
 *   trim         Haplotype::trim(new padded span) (H:149-236): the location must contain the span; new_start is measured from
 *                hap_loc_start, NOT from hap_start_wrt_ref; get_bases_covering_ref_interval (U:759-843) with the start test in
 *                front of the end test inside an M element, a deletion failing on either bound (CUT_IN_DELETION), an insertion
 *                at the cut left out, the two tests behind the loop, min(stop + 1, len); no bases: EMPTY;
 *                trim_cigar_by_reference (U:334-386, :853) through a builder that strips deletions at the ends; a leading or
 *                trailing insertion of the result removed through a builder that does not; nothing left: ALL_INSERTION;
 *                out_hap_start_wrt_ref = new_start + hap_start_wrt_ref.  The bases come out upper-cased (Haplotype::new,
 *                src/model/byte_array_allele.rs:76), and equality and order below are of the upper-cased bytes.  The INPUT
 *                bases are taken as given, as phmm_discover_events takes them: the event map compares raw bytes, so a lower-case
 *                haplotype base against the same base in upper case in the reference is an event whose alleles collapse
 *                (PHMM_EV_STATUS_ALLELES) where the reference, whose haplotypes are upper-cased when they are made, sees no
 *                event.  A caller that may hold lower-case bases upper-cases haplotypes and reference first
 *   panics       where the reference panics or returns Err the region's status is that of its FIRST such haplotype in input
 *                order, the spans and PHMM_TRIM_VARIATION_SPAN stay, it has no output haplotypes, and no other region is
 *                touched: PHMM_TRIM_STATUS_LOCATION  the location does not contain the span (H:159-163);  _LENGTH  bases and
 *                CIGAR disagree (U:772-779);  _OPERATOR  the walk reaches an S (U:818-820; N, H and P fail the event map
 *                first);  _NOT_FOUND  "Never found start or stop" (U:833-838; the CIGAR ends in front of the span);  _BUILDER
 *                a CigarBuilder Err (U:374-377, H:215-222, cigar_builder.rs:321-325): an I behind a right soft clip that sits
 *                just behind the span's end, 10M2S3I cut at its last matched base;  _REF_ELIMINATED  a haplotype with
 *                hap_is_ref that trims to None (S:487-490)
 *   order        trim_down_haplotypes (S:465-499) into a BTreeMap: equality by bases, order by length, then bytes unsigned
 *                (H:269-284).  An equal later haplotype is dropped unless it is a reference haplotype, which replaces key and
 *                value: a class is represented by its LAST member with hap_is_ref, else by its first member in input order, and
 *                the representative's CIGAR, start and is_ref are emitted
 *   variation    PHMM_TRIM_VARIATION_SPAN: the trimmer found variation (T:249-251).  PHMM_TRIM_VARIATION_SET: the result set's
 *                variation_present after trim_to -- some input haplotype is not a reference haplotype (S:340), or some
 *                representative is not (S:411-424); never cleared
 * Inputs, per region: region_ref_off [n_regions+1], ref_bases, region_ref_start, region_hap_off [n_regions+1], hap_off, hap_bases,
 *   hap_cigar_off, hap_cigar ((len << 4) | op), hap_start_wrt_ref, max_mnp_distance as phmm_discover_events takes them;
 *   region_active_start / _end, region_padded_start / _end [n_regions] closed spans, the active one inside the padded one;
 *   hap_loc_start / hap_loc_end [n_haps] the haplotype's genome location, closed;  hap_is_ref [n_haps] bytes;
 *   padding [4]  SNP, indel and STR padding (the reference's defaults: 20, 75, 75) and max_extension_into_region_padding.  The
 *                last two are carried for the ABI: the STR arm has no input (above), the legacy trimmer is not part of this call
 * Outputs, per region [n_regions]: region_status (0, PHMM_EV_STATUS_*, PHMM_TRIM_STATUS_*); variation_present (PHMM_TRIM_VARIATION_*);
 *   variant_start / _end, padded_start / _end the trimmer's two spans; new_active_start / _end, new_padded_start / _end;
 *   out_region_ref_hap  the output haplotype, counted inside the region, that trim_to leaves as ref_haplotype (the last with
 *                is_ref in the map's order), -1 without one
 * per input haplotype [n_haps]: hap_fate  the rank it got inside its region (>= 0), or PHMM_TRIM_FATE_DUPLICATE with hap_dup_of =
 *   its class's representative (counted inside the region; UINT32_MAX otherwise), _CUT_IN_DELETION, _EMPTY, _ALL_INSERTION, or
 *   _NOT_TRIMMED (its region has no variation or a negative status)
 * the trimmed haplotypes, dense, regions in order, inside a region in the BTreeMap's order: out_region_hap_off [n_regions+1],
 *   out_hap_off, out_hap_cigar_off [n_out+1], out_hap_bases, out_hap_cigar, out_hap_start_wrt_ref, out_hap_is_ref [n_out],
 *   out_hap_source [n_out] the input haplotype, counted inside the region.  They pass as they are into phmm_region_compute and
 *   phmm_discover_events; the reference bases and region_ref_start stay the input's (trim_to does not touch
 *   full_reference_with_padding).  Nothing is larger than the input: size the per-haplotype arrays for n_haps (+1 for offsets),
 *   out_hap_bases as hap_bases, out_hap_cigar as hap_cigar; entries behind n_out = out_region_hap_off[n_regions] are not written.
 * Limits as phmm_discover_events: PHMM_EVENTS_MAX_REF reference bases and PHMM_EVENTS_MAX_HAPS haplotypes per region; haplotype
 * bases + CIGAR elements + 8 per haplotype below 2^31.  The device workspace is the one phmm_discover_events keeps.
 * The result is the same from run to run and whatever else is in the batch: no atomics, one writer per element.
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offender): a required array NULL; offsets that do not
 * start at 0 or are not monotonic; a region above a limit; a position beyond 2^62; an active span that is empty or not inside
 * the padded span; a haplotype location that ends before it starts; hap_start_wrt_ref + the location's length beyond 32 bits;
 * a base outside the reference's allele alphabet; a CIGAR element with an unknown operator or length 0.  n_regions == 0 and
 * regions without haplotypes are fine.  One thread per handle.
 */
#define PHMM_TRIM_VARIATION_SPAN 1u
#define PHMM_TRIM_VARIATION_SET 2u
#define PHMM_TRIM_FATE_DUPLICATE (-1)
#define PHMM_TRIM_FATE_CUT_IN_DELETION (-2)
#define PHMM_TRIM_FATE_EMPTY (-3)
#define PHMM_TRIM_FATE_ALL_INSERTION (-4)
#define PHMM_TRIM_FATE_NOT_TRIMMED (-5)
#define PHMM_TRIM_STATUS_LOCATION (-16)
#define PHMM_TRIM_STATUS_LENGTH (-17)
#define PHMM_TRIM_STATUS_OPERATOR (-18)
#define PHMM_TRIM_STATUS_NOT_FOUND (-19)
#define PHMM_TRIM_STATUS_BUILDER (-20)
#define PHMM_TRIM_STATUS_REF_ELIMINATED (-21)
#define PHMM_TRIM_STATUS_REPEAT_SLICE (-22)
int phmm_trim_regions(phmm_handle *h, uint32_t n_regions, const uint32_t *region_ref_off, const uint8_t *ref_bases,
                      const uint64_t *region_ref_start, const uint64_t *region_active_start, const uint64_t *region_active_end,
                      const uint64_t *region_padded_start, const uint64_t *region_padded_end, const uint32_t *region_hap_off,
                      const uint32_t *hap_off, const uint8_t *hap_bases, const uint32_t *hap_cigar_off, const uint32_t *hap_cigar,
                      const uint32_t *hap_start_wrt_ref, const uint64_t *hap_loc_start, const uint64_t *hap_loc_end,
                      const uint8_t *hap_is_ref, uint32_t max_mnp_distance, const uint32_t *padding, int32_t *region_status,
                      uint8_t *variation_present, uint64_t *variant_start, uint64_t *variant_end, uint64_t *padded_start,
                      uint64_t *padded_end, uint64_t *new_active_start, uint64_t *new_active_end, uint64_t *new_padded_start,
                      uint64_t *new_padded_end, int32_t *hap_fate, uint32_t *hap_dup_of, uint32_t *out_region_hap_off,
                      uint32_t *out_hap_off, uint8_t *out_hap_bases, uint32_t *out_hap_cigar_off, uint32_t *out_hap_cigar,
                      uint32_t *out_hap_start_wrt_ref, uint32_t *out_hap_source, uint8_t *out_hap_is_ref,
                      int32_t *out_region_ref_hap);

/*
 * phmm_assembly_regions -- the band-passed state lists of phmm_activity_profile cut into assembly regions, and the staged reads
 * each region's fetch returns, for many profiles in ONE call.  P = src/activity_profile/activity_profile.rs, A =
 * src/assembly/assembly_region.rs, T = src/assembly/assembly_region_iterator.rs, U = src/utils/interval_utils.rs; a profile is
 * made and handed over at src/haplotype/haplotype_caller_engine.rs:947, :982-1136, and popped at
 * src/assembly/assembly_region_walker.rs:124-131.
 * Part A, per profile: pop_ready_assembly_regions (P:371-412) as written, every quirk kept:
 *   force        computed per iteration, the argument ignored (P:384-392): false for the first region, afterwards `the region
 *                before's active start != stop + 1`, stop = region_stop_loc, the position of the last state that was ADDED
 *                (profile_stop), not the end of the band-passed list, which runs up to F states further.  So a list shorter
 *                than max_region_size + max_prob_propagation yields no region at all (P:552-558), and after a region that
 *                happens to start at stop + 1 the next one is unforced and the tail may stay unpopped
 *   boundary     find_first_activity_boundary (P:621-640): `prob > threshold` in f32, a NaN is inactive; bounded by the remaining
 *                states and by max_region_size
 *   cut site     find_best_cut_site (P:582-605) only for an active run that reaches exactly max_region_size: downward from
 *                end - 1 to min_region_size with `cur < min_p && is_minimum(i)`, min_p from f32::MAX: the smallest probability
 *                wins, the HIGHEST index among equals; nothing qualifies: end.  is_minimum (P:660-668) is of the CURRENT list,
 *                after earlier drains: false at its index 0 and at the last state of the whole list, else
 *                p[i] <= p[i+1] && p[i] < p[i-1].  The assertion end >= min_region_size (P:583-586) fails only where it is
 *                reached: PHMM_REG_STATUS_MIN_REGION_SIZE
 *   region       end = min(start + offset, contig length - 1) (P:495-502); region_states = offset + 1 states are drained, which
 *                may be more than the span holds; region_density = #{drained states with prob > 0.05} as f32 / span size as f32
 *                (P:506-508).  A region that would START past contig length - 1 (the list keeps the state AT the contig
 *                length) underflows SimpleInterval::size there: PHMM_REG_STATUS_START_PAST_CONTIG.  Either status ends the
 *                profile at that region: the regions before it stand, other profiles are unaffected
 *   padded span  make_padded_span (A:169-189, U:21-40): saturating start, end min(contig length, end + extension); the None arm
 *                falls back to the active span
 *   Inactive regions are returned too (call_region builds the reference model from them).
 * Part B, skipped when group_read_off is NULL: fill_next_assembly_region_with_reads (T:54-159) without BAM I/O and
 * read_is_filtered.  Per (region, sample) the staged reads a fetch of [padded start, padded end + 1) returns, in input order: the
 * rule is htslib's, pos <= padded end && pos + max(reflen, 1) > padded start with reflen over the CIGAR's M, D, N, = and X
 * elements.  It is htslib's and NOT observable through the reference here: no BAM fixture can be read.  Per read, once:
 * read_mean_qual = sum(qual as f64) / len as f64, the depth cap's key (T:143-147); a read without qualities gives 0 / 0 = NaN.
 * Per region its reads over all samples, and PHMM_REG_OVER_DEPTH where they exceed max_input_depth (T:141).
 * EQUAL to a statement-by-statement restatement, region_density and read_mean_qual bit for bit: each is one correctly rounded
 * division of exactly representable integers.  The same from run to run and whatever the batch: no atomics, one writer per element.
 * Inputs: n_profiles; n_windows and n_samples (the groups of the reads; unused without reads); assembly_region_extension,
 *   min_region_size, max_region_size, max_prob_propagation (the reference's defaults: 100, 50, 300, 50); active_prob_threshold, a
 *   double that holds an f32 value (0.002); max_input_depth;
 *   profile_prob (float) [n_prob] with profile_first / profile_len [n_profiles]: phmm_activity_profile's outputs pass as they
 *   are, profile_first[k] = P_k + k * max_filter_size;  profile_start: the position of state 0;  profile_stop: the position of the
 *   last added state;  profile_contig_length;  profile_window [n_profiles]: the window whose reads are the profile's;
 *   group_read_off [n_windows * n_samples + 1], read_pos, read_cigar_off, read_cigar, read_off, read_quals as
 *   phmm_activity_profile takes them (read_pos must not decrease inside a group)
 * Outputs: profile_status [n_profiles] 0 or PHMM_REG_STATUS_*; profile_region_off [n_profiles+1];
 *   per region: region_start / _end, region_padded_start / _end (closed), region_states, region_flags (PHMM_REG_ACTIVE,
 *   PHMM_REG_FORCED: popped under force, PHMM_REG_OVER_DEPTH), region_density (float), region_n_reads;
 *   region_read_off [n_regions * n_samples + 1] / region_reads: per (region, sample) at region * n_samples + sample the global
 *   indices of its reads;  read_mean_qual [n_reads], may be NULL
 * capacity [2] / required [2] count regions and membership entries, as phmm_discover_events does: when a capacity is too small
 * the call returns PHMM_ERR_EVENT_CAPACITY with `required` filled and nothing else written; all capacities 0 is the cheap way
 * to ask, and the per-region and membership arrays may then be NULL.
 * Out of scope, the caller's: the depth cap's stable sort and take(n) (T:142-150) and the final par_sort_unstable by
 * BirdToolRead::cmp (T:157) -- they need qnames, flags and mates and apply to few regions; read_is_filtered; the assembly graph.
 * PHMM_ERR_INVALID_ARG (nothing written; phmm_last_error names the first offender): min_region_size or max_region_size 0 (the
 * reference asserts both); a required array NULL; profile_first + profile_len past profile_prob; a contig length of 0; a window
 * index out of range; offsets that do not start at 0 or are not monotonic; read_pos negative or smaller than that of the read
 * before it in its group; a CIGAR operator above 8; a position from 2^62 on; reads without samples; states x samples or
 * windows x samples from 2^31 on.  n_profiles == 0 (required = {0, 0}, the offset arrays hold their 0, nothing else is
 * written), empty lists and groups without reads are fine.  One thread per handle.
 */
#define PHMM_REG_ACTIVE 1u
#define PHMM_REG_FORCED 2u
#define PHMM_REG_OVER_DEPTH 4u
#define PHMM_REG_STATUS_MIN_REGION_SIZE (-1)
#define PHMM_REG_STATUS_START_PAST_CONTIG (-2)
int phmm_assembly_regions(phmm_handle *h, uint32_t n_profiles, uint32_t n_windows, uint32_t n_samples,
                          uint32_t assembly_region_extension, uint32_t min_region_size, uint32_t max_region_size,
                          uint32_t max_prob_propagation, double active_prob_threshold, uint32_t max_input_depth, uint32_t n_prob,
                          const void *profile_prob, const uint32_t *profile_first, const uint32_t *profile_len,
                          const uint64_t *profile_start, const uint64_t *profile_stop, const uint64_t *profile_contig_length,
                          const uint32_t *profile_window, const uint32_t *group_read_off, const int64_t *read_pos,
                          const uint32_t *read_cigar_off, const uint32_t *read_cigar, const uint32_t *read_off,
                          const uint8_t *read_quals, const uint32_t *capacity, uint32_t *required, int32_t *profile_status,
                          uint32_t *profile_region_off, uint64_t *region_start, uint64_t *region_end,
                          uint64_t *region_padded_start, uint64_t *region_padded_end, uint32_t *region_states,
                          uint32_t *region_flags, void *region_density, uint32_t *region_n_reads, uint32_t *region_read_off,
                          uint32_t *region_reads, double *read_mean_qual);

/*
 * Developer switches and counters (tests, A/B measurements; never needed in production, NOTEBOOK.md section 11).
 * The PHMM_* environment variables of the same names (upper case) are read once, by phmm_create; phmm_set_switch changes one
 * switch of one handle afterwards.  What is left of them after round 6 (every switch whose A/B was closed went with its code):
 *   planner        "force_L" (16 / 32 / 64 lanes per pair), "force_chain" (reads per run of the chained kernel; 0 = per-read kernel
 *                  only), "force_streams", "no_pipeline" (a host-buffer call in one shot whatever its size), "no_rescue", "trace"
 *   aligner        "sw_lite" (the tags-only first pass: -1 where it pays, 0 never, 1 always), "sw_chunks", "sw_lanes",
 *                  "sw_transpose", "sw_no_zero_copy", "sw_clock"
 *   region call    "region_server" (the resident region server: -1 the one-shot calls of private handles past five alive on the
 *                  device, 0 never, 1 every call its limits admit), "server_idle_us", "server_trace";
 *                  "region_sw_all" (pairs up to which a lone launched call aligns every read against every haplotype beside the
 *                  PairHMM kernels: -1 by load, 0 never), "region_flag_wait", "region_pick_timeout_us", "region_debug_pick" (tests),
 *                  "mirror_canary", "region_own_queue" (environment only)
 *   assembly       "asm_fingerprint_bits" (tests: the bits phmm_assembly_kmers and phmm_assembly_graph keep of a fingerprint, 0 = all 64)
 *   many callers   "route_shared" (opt-in: private handles' small calls through the shared combiner)
 * Value -1 / 0 = back to the planner's choice as documented there.  Not to be called while another thread computes on the handle.
 * Returns PHMM_ERR_INVALID_ARG for an unknown name.
 * phmm_get_stat: "staged_bytes" (payload bytes this handle -- for a shared handle, its lanes -- copied into pinned
 * staging so far), "rescue_passes" (batches that needed the exact pass below -600), "sw_kernel_us" / "sw_backtrack_bytes" /
 * "sw_clock_mhz" (device time of the last phmm_sw_align's kernels by HIP events, the backtrack bytes they stored, the shader
 * clock one of their blocks saw), "sw_second_pass" (alignments of the last aligner call whose walk met a gap behind the
 * tags-only sweep and which the full instance aligned again; 0 when the call took one pass), "sw_instance" (which compiled
 * aligner kernel the first launch of the last phmm_sw_align / _indexed / phmm_realign_* / phmm_calculate_cigar call was: columns
 * -- rows, for the sweep along the alternate -- per lane K in bits 0-7, lanes per alignment L in bits 8-15, bit 16 = the sweep
 * along the alternate, bits 17-19 = variant (1 wide weights | 2 rows in device memory | 4 the tags-only first pass), bits 32-63 =
 * strips of L x K columns; phmm_region_compute's own launches do not set it), "sw_instance_second" (the same for the second pass
 * of that call: the instance that redid the first of its lists of alignments with gaps, 0 when none was redone; decoder:
 * lorikeet_amd/smith_waterman.py decode_instance), "region_sw_all" (region calls that aligned every pair beside the PairHMM
 * kernels so far), "server_jobs" / "server_launches" / "server_broken" (the device's region server: calls it has taken, times it
 * was launched, whether it gave up); unknown names give 0.
 */
int phmm_set_switch(phmm_handle *h, const char *name, int value);
uint64_t phmm_get_stat(phmm_handle *h, const char *name);
/* Developer runs (switch "server_trace" / PHMM_SERVER_TRACE=1): the tasks the device's region server has run since its last
 * launch, one record each -- {u32 sequence number of the call, u32 kind (0 stage-in, 1 a read's chain), u32 index, u32 worker,
 * u64 claimed, u64 begun, u64 ended, u64[4] inside a chain: pre-step done, PairHMM done, post-step done, aligner done} in ticks
 * of the device's 100 MHz clock.  Copies up to `cap` records (72 bytes each) into `out`, returns how many exist; waits for
 * the server to leave the chip first.  tools/server_trace.cpp prints a call's timeline from it. */
uint32_t phmm_server_trace(int device_id, void *out, uint32_t cap);

/* What the library was built from: "activity=<hash> asm=<hash> cigar=<hash> events=<hash> finalize=<hash> genotype=<hash> pairhmm=<hash> phase=<hash> server=<hash> sw=<hash>", the hashes of the kernel sources of each
 * family (tools/source_hash.py) at compile time.  smoke() and bench.py compare it with the tree they run in. */
const char *phmm_build_info(void);

/* Host copies of the device tables, for parity tests against the oracle:
 * eps[q] = 10^(-q/10) for q in 0..=255, mm = triangular match->match table incl. row 255. */
size_t phmm_table_eps(const double **eps);
size_t phmm_table_match_to_match(const double **mm);
/* JacobianLogTable (src/utils/math_utils.rs:9-14, :481-498): log10(1 + 10^(-k * 1e-4)) for k in 0..=80 000, the table
 * phmm_genotype_likelihoods uses on the device */
size_t phmm_table_jacobian(const double **table);

#ifdef __cplusplus
}
#endif
#endif /* PHMM_H */
