//! Safe side of the MI355X PairHMM binding: flattens the data `PairHMM::compute_likelihoods` already holds into the
//! struct-of-arrays `phmm_compute` takes (include/phmm.h) and turns a non-zero status into the panic the rest of
//! the PairHMM path uses for violated preconditions.
//!
//! Two kinds of engine handles.  The per-region pipeline (`region_compute`: everything between
//! `compute_read_likelihoods` and `change_evidence`) goes through ONE shared handle per device with
//! `phmm_region_submit` / `phmm_wait`, so that the regions of all rayon workers waiting at a moment are computed as one
//! batch.  The single-step entry points (`compute_likelihoods`, `realign_reads`, `calculate_cigars`) use one private
//! handle per rayon worker: Lorikeet clones its likelihood engine per region task
//! (src/assembly/assembly_region_walker.rs) and calls synchronously from every worker, and such a handle must not be
//! shared between threads.  Workers are spread over the visible devices round-robin.
use std::cell::RefCell;
use std::ffi::CStr;
use std::sync::atomic::{AtomicU32, Ordering};

use crate::pair_hmm::hip_ffi::*;

/// Flags every engine of this process is created with (`phmm_create`, include/phmm.h).
static ENGINE_FLAGS: AtomicU32 = AtomicU32::new(0);

/// `--pairhmm-backend hip-f32`: engines compute in f32 first (state scaled by 2^120) and redo in f64 what underflows --
/// the arithmetic of the reference's production arm (gkl's AVX kernel, called at src/pair_hmm/pair_hmm.rs:348-366), within
/// 1e-5 of the scalar arm like that one, and 1.5x the f64 rate.  `--pairhmm-backend hip` is f64 throughout (the scalar
/// arm's arithmetic).  Takes effect for engines created afterwards: `AVXMode::select` calls it before any region is computed.
pub fn set_f32_first(on: bool) {
    if on {
        ENGINE_FLAGS.fetch_or(PHMM_FLAG_F32_FIRST as u32, Ordering::Relaxed);
    } else {
        ENGINE_FLAGS.fetch_and(!(PHMM_FLAG_F32_FIRST as u32), Ordering::Relaxed);
    }
}

/// ... or LORIKEET_HIP_F32_FIRST=1 in the environment (read when an engine is created), for runs that cannot change the
/// command line.
fn engine_flags() -> std::os::raw::c_uint {
    let mut flags = ENGINE_FLAGS.load(Ordering::Relaxed);
    if std::env::var("LORIKEET_HIP_F32_FIRST").map(|v| !v.is_empty() && v != "0").unwrap_or(false) {
        flags |= PHMM_FLAG_F32_FIRST as u32;
    }
    flags as std::os::raw::c_uint
}

struct Engine(*mut phmm_handle);

impl Drop for Engine {
    fn drop(&mut self) {
        unsafe { phmm_destroy(self.0) }
    }
}

thread_local! {
    static ENGINE: RefCell<Option<Engine>> = RefCell::new(None);
}

/// Number of MI355X devices the process can use (0: the backend is unavailable).
pub fn device_count() -> i32 {
    unsafe { phmm_device_count() }
}

fn last_error(h: *mut phmm_handle) -> String {
    unsafe { CStr::from_ptr(phmm_last_error(h)).to_string_lossy().into_owned() }
}

fn with_engine<R>(f: impl FnOnce(*mut phmm_handle) -> R) -> R {
    ENGINE.with(|cell| {
        let mut slot = cell.borrow_mut();
        if slot.is_none() {
            let n = device_count().max(1);
            let device = (rayon::current_thread_index().unwrap_or(0) as i32) % n;
            let h = unsafe { phmm_create(device, engine_flags()) };
            if h.is_null() {
                panic!("HIP PairHMM: {}", last_error(std::ptr::null_mut()));
            }
            *slot = Some(Engine(h));
        }
        f(slot.as_ref().unwrap().0)
    })
}

/// log10 Pr(read | haplotype) for every read x haplotype of one region: read-major, haplotypes in list order --
/// the layout of `PairHMM::m_log_likelihood_array`.
pub fn compute_likelihoods(
    haplotypes: &[&[u8]],
    read_bases: &[&[u8]],
    read_quals: &[&[u8]],
    insertion_gop: &[&[u8]],
    deletion_gop: &[&[u8]],
    overall_gcp: &[&[u8]],
) -> Vec<f64> {
    let n_reads = read_bases.len();
    let n_haps = haplotypes.len();
    let mut read_off: Vec<u32> = Vec::with_capacity(n_reads + 1);
    read_off.push(0);
    let total: usize = read_bases.iter().map(|r| r.len()).sum();
    let (mut bases, mut quals, mut ins, mut del, mut gcp) = (
        Vec::with_capacity(total),
        Vec::with_capacity(total),
        Vec::with_capacity(total),
        Vec::with_capacity(total),
        Vec::with_capacity(total),
    );
    for r in 0..n_reads {
        let n = read_bases[r].len();
        assert!(
            read_quals[r].len() == n && insertion_gop[r].len() == n && deletion_gop[r].len() == n && overall_gcp[r].len() == n,
            "Read bases and read quals aren't the same size"
        );
        bases.extend_from_slice(read_bases[r]);
        quals.extend_from_slice(read_quals[r]);
        ins.extend_from_slice(insertion_gop[r]);
        del.extend_from_slice(deletion_gop[r]);
        gcp.extend_from_slice(overall_gcp[r]);
        read_off.push(bases.len() as u32);
    }
    let mut hap_off: Vec<u32> = Vec::with_capacity(n_haps + 1);
    hap_off.push(0);
    let mut haps: Vec<u8> = Vec::with_capacity(haplotypes.iter().map(|h| h.len()).sum());
    for h in haplotypes {
        haps.extend_from_slice(h);
        hap_off.push(haps.len() as u32);
    }
    let mut out = vec![0.0f64; n_reads * n_haps];
    let region_read_off = [0u32, n_reads as u32];
    let region_hap_off = [0u32, n_haps as u32];
    let out_off = [0u64, (n_reads * n_haps) as u64];
    with_engine(|h| {
        let rc = unsafe {
            phmm_compute(
                h,
                1,
                region_read_off.as_ptr(),
                region_hap_off.as_ptr(),
                read_off.as_ptr(),
                bases.as_ptr(),
                quals.as_ptr(),
                ins.as_ptr(),
                del.as_ptr(),
                gcp.as_ptr(),
                hap_off.as_ptr(),
                haps.as_ptr(),
                out_off.as_ptr(),
                out.as_mut_ptr(),
            )
        };
        if rc != PHMM_OK {
            // the scalar arm asserts the same conditions (pair_hmm.rs: argument sizes, result <= 0)
            panic!("HIP PairHMM failed ({}): {}", rc, last_error(h));
        }
    });
    out
}

/// One unit of evidence after `realign_to_best`: `AlleleLikelihoods::BestAllele` (allele index, likelihood,
/// confidence) and the read's Smith-Waterman alignment to that haplotype (BAM-encoded CIGAR elements,
/// `(length << 4) | op`, and `SmithWatermanAlignmentResult::alignment_offset`).  `allele_index` is `None`, and the
/// CIGAR empty, where the reference has no best allele for the read.
pub struct RealignedToBest {
    pub allele_index: Option<usize>,
    pub likelihood: f64,
    pub confidence: f64,
    pub cigar: Vec<u32>,
    pub alignment_offset: i32,
}

/// The arithmetic of `AssemblyBasedCallerUtils::realign_reads_to_their_best_haplotype`
/// (src/assembly/assembly_based_caller_utils.rs:208-246) for one region in one call: the best allele of every read
/// with ties broken by `priorities` (`AlleleLikelihoods::best_alleles_breaking_ties_main`,
/// src/model/allele_likelihoods.rs:1043-1095) and the read's alignment to that haplotype with
/// `ALIGNMENT_TO_BEST_HAPLOTYPE_SW_PARAMETERS` and `OverhangStrategy::SoftClip`
/// (src/reads/alignment_utils.rs:52-58).  `likelihoods` is read-major (`[read][haplotype]`, what
/// `compute_likelihoods` above returns); `reads_minus_soft_clips` are the hard-clipped reads of
/// alignment_utils.rs:47-50; `priorities` one value per haplotype
/// (`haplotype_alignment_tiebreaking_priority`, assembly_based_caller_utils.rs:187-195).
pub fn realign_to_best(
    haplotypes: &[&[u8]],
    reads_minus_soft_clips: &[&[u8]],
    likelihoods: &[f64],
    priorities: &[i32],
) -> Vec<RealignedToBest> {
    let n_reads = reads_minus_soft_clips.len();
    let n_haps = haplotypes.len();
    assert!(likelihoods.len() == n_reads * n_haps && priorities.len() == n_haps, "one likelihood per read and haplotype, one priority per haplotype");
    let mut read_off: Vec<u32> = Vec::with_capacity(n_reads + 1);
    read_off.push(0);
    let mut bases: Vec<u8> = Vec::with_capacity(reads_minus_soft_clips.iter().map(|r| r.len()).sum());
    for r in reads_minus_soft_clips {
        bases.extend_from_slice(r);
        read_off.push(bases.len() as u32);
    }
    let mut hap_off: Vec<u32> = Vec::with_capacity(n_haps + 1);
    hap_off.push(0);
    let mut haps: Vec<u8> = Vec::with_capacity(haplotypes.iter().map(|h| h.len()).sum());
    for h in haplotypes {
        haps.extend_from_slice(h);
        hap_off.push(haps.len() as u32);
    }
    let region_read_off = [0u32, n_reads as u32];
    let region_hap_off = [0u32, n_haps as u32];
    let out_off = [0u64, (n_reads * n_haps) as u64];
    // ALIGNMENT_TO_BEST_HAPLOTYPE_SW_PARAMETERS (src/smith_waterman/smith_waterman_aligner.rs:23-26)
    let params = phmm_sw_parameters { match_value: 10, mismatch_penalty: -15, gap_open_penalty: -30, gap_extend_penalty: -5 };
    let mut capacity = vec![16u64; n_reads];
    let mut best = vec![0i32; n_reads];
    let mut likelihood = vec![0.0f64; n_reads];
    let mut confidence = vec![0.0f64; n_reads];
    let mut n_cigar = vec![0u32; n_reads];
    let mut offset = vec![0i32; n_reads];
    let mut cigar_off = vec![0u64; n_reads + 1];
    let mut cigar: Vec<u32> = Vec::new();
    with_engine(|h| {
        for attempt in 0..2 {
            for r in 0..n_reads {
                cigar_off[r + 1] = cigar_off[r] + capacity[r];
            }
            cigar = vec![0u32; cigar_off[n_reads] as usize];
            let rc = unsafe {
                phmm_realign_to_best(
                    h,
                    1,
                    region_read_off.as_ptr(),
                    region_hap_off.as_ptr(),
                    read_off.as_ptr(),
                    bases.as_ptr(),
                    hap_off.as_ptr(),
                    haps.as_ptr(),
                    out_off.as_ptr(),
                    likelihoods.as_ptr(),
                    std::ptr::null(),
                    priorities.as_ptr(),
                    0.2, // LOG_10_INFORMATIVE_THRESHOLD (src/model/allele_likelihoods.rs:17)
                    &params,
                    PHMM_SW_SOFTCLIP,
                    cigar_off.as_ptr(),
                    cigar.as_mut_ptr(),
                    n_cigar.as_mut_ptr(),
                    offset.as_mut_ptr(),
                    best.as_mut_ptr(),
                    likelihood.as_mut_ptr(),
                    confidence.as_mut_ptr(),
                )
            };
            if rc == PHMM_ERR_CIGAR_CAPACITY && attempt == 0 {
                // the library reports the sizes: once more with those
                for r in 0..n_reads {
                    capacity[r] = capacity[r].max(n_cigar[r] as u64);
                }
                continue;
            }
            if rc != PHMM_OK {
                panic!("HIP realignment failed ({}): {}", rc, last_error(h));
            }
            break;
        }
    });
    (0..n_reads)
        .map(|r| {
            let start = cigar_off[r] as usize;
            RealignedToBest {
                allele_index: if best[r] >= 0 { Some(best[r] as usize) } else { None },
                likelihood: likelihood[r],
                confidence: confidence[r],
                cigar: cigar[start..start + n_cigar[r] as usize].to_vec(),
                alignment_offset: offset[r],
            }
        })
        .collect()
}

/// One read after `realign_reads`: its `BestAllele` and, when `realigned`, the position and CIGAR
/// `AlignmentUtils::create_read_aligned_to_ref` would give it (BAM-encoded elements, clips of the original CIGAR
/// included).  `realigned == false`: the reference returns the read unchanged (no best allele, or
/// `alignment_offset == -1`, src/reads/alignment_utils.rs:60-63).
pub struct RealignedRead {
    pub allele_index: Option<usize>,
    pub likelihood: f64,
    pub confidence: f64,
    pub realigned: bool,
    pub pos: i64,
    pub cigar: Vec<u32>,
}

/// `AssemblyBasedCallerUtils::realign_reads_to_their_best_haplotype`
/// (src/assembly/assembly_based_caller_utils.rs:208-246) for one region in one call of the library: best alleles,
/// the reads' alignments to them and `create_read_aligned_to_ref`'s projection onto the reference
/// (src/reads/alignment_utils.rs:83-165).  `haplotype_cigars[a]` / `alignment_start_hap_wrt_ref[a]` are
/// `Haplotype::cigar` / `alignment_start_hap_wrt_ref` of haplotype `a`, `reference_haplotype` its index,
/// `reference_start` is `padded_reference_loc.get_start()`, `original_cigars[r]` the read's CIGAR before realignment.
/// Panics where the reference panics ("Read goes past end of reference", builder errors ...).
#[allow(clippy::too_many_arguments)]
pub fn realign_reads(
    haplotypes: &[&[u8]],
    haplotype_cigars: &[&[u32]],
    alignment_start_hap_wrt_ref: &[u32],
    reference_haplotype: usize,
    reference_start: u64,
    reads_minus_soft_clips: &[&[u8]],
    original_cigars: &[&[u32]],
    likelihoods: &[f64],
    priorities: &[i32],
) -> Vec<RealignedRead> {
    let n_reads = reads_minus_soft_clips.len();
    let n_haps = haplotypes.len();
    assert!(likelihoods.len() == n_reads * n_haps && priorities.len() == n_haps, "one likelihood per read and haplotype, one priority per haplotype");
    assert!(haplotype_cigars.len() == n_haps && alignment_start_hap_wrt_ref.len() == n_haps && original_cigars.len() == n_reads);
    let flatten_u8 = |parts: &[&[u8]]| {
        let mut off: Vec<u32> = vec![0];
        let mut all: Vec<u8> = Vec::new();
        for p in parts {
            all.extend_from_slice(p);
            off.push(all.len() as u32);
        }
        (off, all)
    };
    let flatten_u32 = |parts: &[&[u32]]| {
        let mut off: Vec<u32> = vec![0];
        let mut all: Vec<u32> = Vec::new();
        for p in parts {
            all.extend_from_slice(p);
            off.push(all.len() as u32);
        }
        (off, all)
    };
    let (read_off, bases) = flatten_u8(reads_minus_soft_clips);
    let (hap_off, haps) = flatten_u8(haplotypes);
    let (hap_cigar_off, hap_cigar) = flatten_u32(haplotype_cigars);
    let (orig_cigar_off, orig_cigar) = flatten_u32(original_cigars);
    let region_read_off = [0u32, n_reads as u32];
    let region_hap_off = [0u32, n_haps as u32];
    let out_off = [0u64, (n_reads * n_haps) as u64];
    let region_ref_hap = [reference_haplotype as i32];
    let region_reference_start = [reference_start];
    let params = phmm_sw_parameters { match_value: 10, mismatch_penalty: -15, gap_open_penalty: -30, gap_extend_penalty: -5 };
    let mut capacity = vec![16u64; n_reads];
    let mut best = vec![0i32; n_reads];
    let mut likelihood = vec![0.0f64; n_reads];
    let mut confidence = vec![0.0f64; n_reads];
    let mut n_out = vec![0u32; n_reads];
    let mut pos = vec![0i64; n_reads];
    let mut status = vec![0i32; n_reads];
    let mut out_cigar_off = vec![0u64; n_reads + 1];
    let mut out_cigar: Vec<u32> = Vec::new();
    with_engine(|h| {
        for attempt in 0..2 {
            for r in 0..n_reads {
                out_cigar_off[r + 1] = out_cigar_off[r] + capacity[r];
            }
            out_cigar = vec![0u32; out_cigar_off[n_reads] as usize];
            let rc = unsafe {
                phmm_realign_reads(
                    h,
                    1,
                    region_read_off.as_ptr(),
                    region_hap_off.as_ptr(),
                    read_off.as_ptr(),
                    bases.as_ptr(),
                    hap_off.as_ptr(),
                    haps.as_ptr(),
                    out_off.as_ptr(),
                    likelihoods.as_ptr(),
                    std::ptr::null(),
                    priorities.as_ptr(),
                    0.2,
                    &params,
                    PHMM_SW_SOFTCLIP,
                    region_ref_hap.as_ptr(),
                    region_reference_start.as_ptr(),
                    hap_cigar_off.as_ptr(),
                    hap_cigar.as_ptr(),
                    alignment_start_hap_wrt_ref.as_ptr(),
                    orig_cigar_off.as_ptr(),
                    orig_cigar.as_ptr(),
                    out_cigar_off.as_ptr(),
                    out_cigar.as_mut_ptr(),
                    n_out.as_mut_ptr(),
                    pos.as_mut_ptr(),
                    status.as_mut_ptr(),
                    best.as_mut_ptr(),
                    likelihood.as_mut_ptr(),
                    confidence.as_mut_ptr(),
                )
            };
            if rc == PHMM_ERR_CIGAR_CAPACITY && attempt == 0 {
                for r in 0..n_reads {
                    capacity[r] = capacity[r].max(n_out[r] as u64);
                }
                continue;
            }
            if rc != PHMM_OK {
                panic!("HIP realignment failed ({}): {}", rc, last_error(h));
            }
            break;
        }
    });
    (0..n_reads)
        .map(|r| {
            if status[r] < 0 {
                // the reference panics on this read (builder error, read past the end of the reference, ...)
                panic!("Failed to realign read {} (status {})", r, status[r]);
            }
            let start = out_cigar_off[r] as usize;
            RealignedRead {
                allele_index: if best[r] >= 0 { Some(best[r] as usize) } else { None },
                likelihood: likelihood[r],
                confidence: confidence[r],
                realigned: status[r] == PHMM_PROJECT_REALIGNED,
                pos: pos[r],
                cigar: out_cigar[start..start + n_out[r] as usize].to_vec(),
            }
        })
        .collect()
}

// ---- the whole per-region path in one call (phmm_region_submit / phmm_wait on ONE shared handle) ----------------------

/// BAM encoding of a CIGAR: `(length << 4) | op`, M = 0, I = 1, D = 2, N = 3, S = 4, H = 5, P = 6, `=` = 7, X = 8.
pub fn encode_cigar(cigar: &[rust_htslib::bam::record::Cigar]) -> Vec<u32> {
    use rust_htslib::bam::record::Cigar;
    cigar
        .iter()
        .map(|c| {
            let op = match c {
                Cigar::Match(_) => 0u32,
                Cigar::Ins(_) => 1,
                Cigar::Del(_) => 2,
                Cigar::RefSkip(_) => 3,
                Cigar::SoftClip(_) => 4,
                Cigar::HardClip(_) => 5,
                Cigar::Pad(_) => 6,
                Cigar::Equal(_) => 7,
                Cigar::Diff(_) => 8,
            };
            (c.len() << 4) | op
        })
        .collect()
}

/// The inverse of `encode_cigar`.
pub fn decode_cigar(elements: &[u32]) -> rust_htslib::bam::record::CigarString {
    use rust_htslib::bam::record::{Cigar, CigarString};
    CigarString(
        elements
            .iter()
            .map(|e| {
                let len = e >> 4;
                match e & 0xf {
                    0 => Cigar::Match(len),
                    1 => Cigar::Ins(len),
                    2 => Cigar::Del(len),
                    3 => Cigar::RefSkip(len),
                    4 => Cigar::SoftClip(len),
                    5 => Cigar::HardClip(len),
                    6 => Cigar::Pad(len),
                    7 => Cigar::Equal(len),
                    8 => Cigar::Diff(len),
                    other => panic!("Unknown CIGAR operator code {}", other),
                }
            })
            .collect(),
    )
}

/// (leading, trailing) soft-clipped bases of a read: what `ReadClipper::hard_clip_soft_clipped_bases`
/// (src/reads/read_clipper.rs:395-435) cuts off its two ends.
pub fn soft_clips(cigar: &[rust_htslib::bam::record::Cigar]) -> (u32, u32) {
    use rust_htslib::bam::record::Cigar;
    let (mut lead, mut trail, mut right_tail) = (0u32, 0u32, false);
    for c in cigar {
        match c {
            Cigar::SoftClip(n) => {
                if right_tail {
                    trail += *n;
                } else {
                    lead += *n;
                }
            }
            Cigar::HardClip(_) => {}
            _ => {
                right_tail = true;
                trail = 0;
            }
        }
    }
    (lead, trail)
}

struct Shared(Vec<*mut phmm_handle>);
// phmm_submit / phmm_region_submit / phmm_wait are the entry points of the library that any number of threads may call
// on one handle (include/phmm.h)
unsafe impl Send for Shared {}
unsafe impl Sync for Shared {}

lazy_static! {
    /// One engine per device for ALL rayon workers: a worker's region is only queued, and the first worker that waits
    /// while an engine lane is free computes the regions of every worker waiting at that moment as ONE batch and hands
    /// each its results (include/phmm.h, phmm_submit).  Lorikeet's call pattern -- one region per call from every
    /// worker, src/assembly/assembly_region_walker.rs:210-273 -- then fills the device instead of a fraction of it.
    static ref SHARED: Shared = {
        let n = device_count().max(1);
        Shared(
            (0..n)
                .map(|device| {
                    let h = unsafe { phmm_create(device, engine_flags()) };
                    if h.is_null() {
                        panic!("HIP PairHMM: {}", last_error(std::ptr::null_mut()));
                    }
                    h
                })
                .collect(),
        )
    };
}

/// The shared engine of this worker's device (workers are spread over the visible devices round-robin).
fn shared_engine() -> *mut phmm_handle {
    let handles = &SHARED.0;
    handles[rayon::current_thread_index().unwrap_or(0) % handles.len()]
}

/// What `PairHMMLikelihoodCalculationEngine::compute_read_likelihoods` and
/// `AssemblyBasedCallerUtils::realign_reads_to_their_best_haplotype` produce together for one region.
pub struct RegionOutput {
    /// normalised log10 likelihoods, read-major (`[read][haplotype]`)
    pub likelihoods: Vec<f64>,
    /// `false`: `filter_poorly_modeled_evidence` removes the read (src/model/allele_likelihoods.rs:925-964)
    pub keep: Vec<bool>,
    /// per read: `BestAllele` and the realigned position / CIGAR (`realigned == false` for removed reads)
    pub reads: Vec<RealignedRead>,
}

/// One call for everything `HaplotypeCallerEngine::call_region` does with numbers between
/// `compute_read_likelihoods` and `change_evidence` (src/haplotype/haplotype_caller_engine.rs:1311-1357): the PCR
/// indel model and quality caps (`modify_read_qualities`), the PairHMM, `normalize_likelihoods`, the keep / remove
/// decision of `filter_poorly_modeled_evidence`, the best allele of every surviving read with
/// `haplotype_alignment_tiebreaking_priority`, its Smith-Waterman alignment to that haplotype and
/// `create_read_aligned_to_ref`'s projection onto the reference.  The likelihood matrix never leaves the device in
/// between.  `read_quals` / `ins_quals` / `del_quals` are the ORIGINAL qualities of what the PairHMM sees
/// (`read.qual()`, BI / BD or the flat Q45 default), `soft_clips[r]` the (leading, trailing) soft-clipped bases
/// inside `read_bases[r]` (all zero when the reads were hard-clipped beforehand), `cfg` the engine's parameters.
#[allow(clippy::too_many_arguments)]
pub fn region_compute(
    cfg: &phmm_engine_config,
    haplotypes: &[&[u8]],
    haplotype_cigars: &[Vec<u32>],
    alignment_start_hap_wrt_ref: &[u32],
    reference_haplotype: usize,
    reference_start: u64,
    priorities: &[i32],
    read_bases: &[&[u8]],
    read_quals: &[&[u8]],
    ins_quals: &[Vec<u8>],
    del_quals: &[Vec<u8>],
    mapq: &[u8],
    soft_clips: &[(u32, u32)],
    original_cigars: &[Vec<u32>],
) -> RegionOutput {
    let n_reads = read_bases.len();
    let n_haps = haplotypes.len();
    assert!(
        read_quals.len() == n_reads && ins_quals.len() == n_reads && del_quals.len() == n_reads && mapq.len() == n_reads
            && soft_clips.len() == n_reads && original_cigars.len() == n_reads,
        "one entry per read"
    );
    assert!(haplotype_cigars.len() == n_haps && alignment_start_hap_wrt_ref.len() == n_haps && priorities.len() == n_haps, "one entry per haplotype");
    let mut read_off: Vec<u32> = vec![0];
    let (mut bases, mut quals, mut ins, mut del) = (Vec::new(), Vec::new(), Vec::new(), Vec::new());
    for r in 0..n_reads {
        let n = read_bases[r].len();
        assert!(read_quals[r].len() == n && ins_quals[r].len() == n && del_quals[r].len() == n, "Read bases and read quals aren't the same size");
        bases.extend_from_slice(read_bases[r]);
        quals.extend_from_slice(read_quals[r]);
        ins.extend_from_slice(&ins_quals[r]);
        del.extend_from_slice(&del_quals[r]);
        read_off.push(bases.len() as u32);
    }
    let mut hap_off: Vec<u32> = vec![0];
    let mut haps: Vec<u8> = Vec::new();
    for h in haplotypes {
        haps.extend_from_slice(h);
        hap_off.push(haps.len() as u32);
    }
    let flatten_u32 = |parts: &[Vec<u32>]| {
        let mut off: Vec<u32> = vec![0];
        let mut all: Vec<u32> = Vec::new();
        for p in parts {
            all.extend_from_slice(p);
            off.push(all.len() as u32);
        }
        (off, all)
    };
    let (hap_cigar_off, hap_cigar) = flatten_u32(haplotype_cigars);
    let (orig_cigar_off, orig_cigar) = flatten_u32(original_cigars);
    let clips: Vec<u32> = soft_clips.iter().flat_map(|c| [c.0, c.1]).collect();
    let any_clip = clips.iter().any(|c| *c != 0);
    let region_read_off = [0u32, n_reads as u32];
    let region_hap_off = [0u32, n_haps as u32];
    let out_off = [0u64, (n_reads * n_haps) as u64];
    let region_ref_hap = [reference_haplotype as i32];
    let region_reference_start = [reference_start];
    let rcfg = phmm_realign_config {
        // ALIGNMENT_TO_BEST_HAPLOTYPE_SW_PARAMETERS, OverhangStrategy::SoftClip (src/reads/alignment_utils.rs:52-58)
        sw_parameters: phmm_sw_parameters { match_value: 10, mismatch_penalty: -15, gap_open_penalty: -30, gap_extend_penalty: -5 },
        overhang_strategy: PHMM_SW_SOFTCLIP,
        // the caller returns before realigning when one allele is left (haplotype_caller_engine.rs:1339-1345)
        flags: PHMM_REGION_SKIP_SINGLE_ALLELE,
        informative_threshold: 0.2, // LOG_10_INFORMATIVE_THRESHOLD (src/model/allele_likelihoods.rs:17)
    };
    let mut likelihoods = vec![0.0f64; n_reads * n_haps];
    let mut keep = vec![0u8; n_reads];
    let mut best = vec![0i32; n_reads];
    let mut likelihood = vec![0.0f64; n_reads];
    let mut confidence = vec![0.0f64; n_reads];
    let mut n_out = vec![0u32; n_reads];
    let mut pos = vec![0i64; n_reads];
    let mut status = vec![0i32; n_reads];
    let mut capacity = vec![16u64; n_reads];
    let mut out_cigar_off = vec![0u64; n_reads + 1];
    let mut out_cigar: Vec<u32> = Vec::new();
    let h = shared_engine();
    for attempt in 0..2 {
        for r in 0..n_reads {
            out_cigar_off[r + 1] = out_cigar_off[r] + capacity[r];
        }
        out_cigar = vec![0u32; out_cigar_off[n_reads] as usize];
        let mut ticket = 0u64;
        let mut rc = unsafe {
            phmm_region_submit(
                h,
                cfg,
                &rcfg,
                1,
                region_read_off.as_ptr(),
                region_hap_off.as_ptr(),
                read_off.as_ptr(),
                bases.as_ptr(),
                quals.as_ptr(),
                ins.as_ptr(),
                del.as_ptr(),
                mapq.as_ptr(),
                if any_clip { clips.as_ptr() } else { std::ptr::null() },
                hap_off.as_ptr(),
                haps.as_ptr(),
                region_ref_hap.as_ptr(),
                out_off.as_ptr(),
                priorities.as_ptr(),
                region_reference_start.as_ptr(),
                hap_cigar_off.as_ptr(),
                hap_cigar.as_ptr(),
                alignment_start_hap_wrt_ref.as_ptr(),
                orig_cigar_off.as_ptr(),
                orig_cigar.as_ptr(),
                out_cigar_off.as_ptr(),
                likelihoods.as_mut_ptr(),
                keep.as_mut_ptr(),
                best.as_mut_ptr(),
                likelihood.as_mut_ptr(),
                confidence.as_mut_ptr(),
                out_cigar.as_mut_ptr(),
                n_out.as_mut_ptr(),
                pos.as_mut_ptr(),
                status.as_mut_ptr(),
                &mut ticket,
            )
        };
        if rc == PHMM_OK {
            // every array above stays alive and untouched until the ticket has been waited for
            rc = unsafe { phmm_wait(h, ticket) };
        }
        if rc == PHMM_ERR_CIGAR_CAPACITY && attempt == 0 {
            for r in 0..n_reads {
                capacity[r] = capacity[r].max(n_out[r] as u64);
            }
            continue;
        }
        if rc != PHMM_OK {
            // the scalar arm asserts the same conditions (argument sizes, result <= 0)
            panic!("HIP region pipeline failed ({}): {}", rc, last_error(h));
        }
        break;
    }
    let reads = (0..n_reads)
        .map(|r| {
            if status[r] < 0 {
                // the reference panics on this read (builder error, read past the end of the reference, ...)
                panic!("Failed to realign read {} (status {})", r, status[r]);
            }
            let start = out_cigar_off[r] as usize;
            RealignedRead {
                allele_index: if best[r] >= 0 { Some(best[r] as usize) } else { None },
                likelihood: likelihood[r],
                confidence: confidence[r],
                realigned: status[r] == PHMM_PROJECT_REALIGNED,
                pos: pos[r],
                cigar: out_cigar[start..start + n_out[r] as usize].to_vec(),
            }
        })
        .collect();
    RegionOutput { likelihoods, keep: keep.iter().map(|k| *k != 0).collect(), reads }
}

/// The realignment half of `region_compute`, carried from `compute_read_likelihoods` to
/// `realign_reads_to_their_best_haplotype`: both run back to back on the same rayon worker
/// (src/haplotype/haplotype_caller_engine.rs:1311-1357), so the token is thread-local, and it names the evidence it
/// belongs to (surviving reads per sample, number of alleles) so that a stale one is never used.
pub struct RegionRealignment {
    pub evidence_counts: Vec<usize>,
    pub n_alleles: usize,
    /// per sample, per surviving read in evidence order
    pub reads: Vec<Vec<RealignedRead>>,
}

thread_local! {
    static REALIGNMENT: RefCell<Option<RegionRealignment>> = RefCell::new(None);
}

pub fn stash_realignment(r: RegionRealignment) {
    REALIGNMENT.with(|cell| *cell.borrow_mut() = Some(r));
}

pub fn clear_realignment() {
    REALIGNMENT.with(|cell| *cell.borrow_mut() = None);
}

/// The stashed result if it belongs to exactly this evidence; consumed either way.
pub fn take_realignment(evidence_counts: &[usize], n_alleles: usize) -> Option<Vec<Vec<RealignedRead>>> {
    REALIGNMENT.with(|cell| match cell.borrow_mut().take() {
        Some(r) if r.evidence_counts.as_slice() == evidence_counts && r.n_alleles == n_alleles => Some(r.reads),
        _ => None,
    })
}

/// `CigarUtils::calculate_cigar` (src/reads/cigar_utils.rs:358-457) for a batch of (reference, haplotype) pairs under
/// one parameter set and one overhang strategy (`PHMM_SW_*`): `None` where the reference returns `None`
/// (`is_s_w_failure`), BAM-encoded elements otherwise.  Panics where the reference panics.
pub fn calculate_cigars(pairs: &[(&[u8], &[u8])], parameters: (i32, i32, i32, i32), overhang_strategy: i32) -> Vec<Option<Vec<u32>>> {
    let n = pairs.len();
    let mut ref_off: Vec<u32> = vec![0];
    let mut alt_off: Vec<u32> = vec![0];
    let (mut refs, mut alts): (Vec<u8>, Vec<u8>) = (Vec::new(), Vec::new());
    for (r, a) in pairs {
        refs.extend_from_slice(r);
        alts.extend_from_slice(a);
        ref_off.push(refs.len() as u32);
        alt_off.push(alts.len() as u32);
    }
    let params = phmm_sw_parameters { match_value: parameters.0, mismatch_penalty: parameters.1, gap_open_penalty: parameters.2, gap_extend_penalty: parameters.3 };
    let mut capacity = vec![16u64; n];
    let mut cigar_off = vec![0u64; n + 1];
    let mut cigar: Vec<u32> = Vec::new();
    let mut n_cigar = vec![0u32; n];
    let mut status = vec![0i32; n];
    with_engine(|h| {
        for attempt in 0..2 {
            for a in 0..n {
                cigar_off[a + 1] = cigar_off[a] + capacity[a];
            }
            cigar = vec![0u32; cigar_off[n] as usize];
            let rc = unsafe {
                phmm_calculate_cigar(
                    h,
                    n as u32,
                    ref_off.as_ptr(),
                    refs.as_ptr(),
                    alt_off.as_ptr(),
                    alts.as_ptr(),
                    &params,
                    overhang_strategy,
                    cigar_off.as_ptr(),
                    cigar.as_mut_ptr(),
                    n_cigar.as_mut_ptr(),
                    status.as_mut_ptr(),
                )
            };
            if rc == PHMM_ERR_CIGAR_CAPACITY && attempt == 0 {
                for a in 0..n {
                    capacity[a] = capacity[a].max(n_cigar[a] as u64);
                }
                continue;
            }
            if rc != PHMM_OK {
                panic!("HIP calculate_cigar failed ({}): {}", rc, last_error(h));
            }
            break;
        }
    });
    (0..n)
        .map(|a| {
            if status[a] < 0 {
                panic!("calculate_cigar: the alignment of pair {} is one the reference panics on (status {})", a, status[a]);
            }
            if status[a] == 1 {
                None
            } else {
                let start = cigar_off[a] as usize;
                Some(cigar[start..start + n_cigar[a] as usize].to_vec())
            }
        })
        .collect()
}

/// One window of `activity_profile`: `outer_chunk_location.start`, the reference bases from there on (the window is as long
/// as they are), the contig's length, and per sample the reads that passed `read_is_filtered`, in fetch order, as
/// (pos, BAM-encoded CIGAR, bases in ASCII, qualities).
pub struct ActivityWindow<'a> {
    pub start: u64,
    pub reference: &'a [u8],
    pub contig_length: u64,
    pub samples: Vec<Vec<(i64, Vec<u32>, &'a [u8], &'a [u8])>>,
}

/// What `activity_profile` returns: per window its status (negative: the reference panics there), then over the positions of
/// all windows in order `depth[position * n_samples + sample]` (ref_depth + non_ref_depth, what the ANI depth runs read), the
/// soft-clip average and is_active_prob, and per profile (`ceil(window length / profile_size)` per window) its band-passed
/// state list -- what `pop_ready_assembly_regions` scans.
pub struct ActivityOutput {
    pub window_status: Vec<i32>,
    pub depth: Vec<u32>,
    pub soft_clip_mean: Vec<f64>,
    pub is_active_prob: Vec<f32>,
    pub profiles: Vec<Vec<f32>>,
}

/// `update_activity_profile` + `calculate_activity_probabilities` up to `BandPassActivityProfile::add`
/// (src/haplotype/haplotype_caller_engine.rs:627-1107) for a batch of windows.  The pseudo counts and `stand_min_conf` are
/// those of the `active_region_evaluation_genotyper_engine`; the band-pass runs at the reference's constants.
pub fn activity_profile(
    windows: &[ActivityWindow],
    n_samples: usize,
    ploidy: usize,
    bq: u8,
    pseudo_counts: (f64, f64, f64),
    stand_min_conf: f64,
    max_prob_propagation: usize,
    profile_size: usize,
) -> ActivityOutput {
    const MAX_FILTER_SIZE: u32 = 50;
    const SIGMA: f64 = 17.0;
    let n = windows.len();
    let window_start: Vec<u64> = windows.iter().map(|w| w.start).collect();
    let window_len: Vec<u32> = windows.iter().map(|w| w.reference.len() as u32).collect();
    let contig_length: Vec<u64> = windows.iter().map(|w| w.contig_length).collect();
    let (mut ref_off, mut group_off, mut cigar_off, mut read_off): (Vec<u32>, Vec<u32>, Vec<u32>, Vec<u32>) = (vec![0], vec![0], vec![0], vec![0]);
    let (mut refs, mut bases, mut quals): (Vec<u8>, Vec<u8>, Vec<u8>) = (Vec::new(), Vec::new(), Vec::new());
    let mut cigars: Vec<u32> = Vec::new();
    let mut read_pos: Vec<i64> = Vec::new();
    for w in windows {
        assert_eq!(w.samples.len(), n_samples, "activity_profile: every window carries every sample");
        refs.extend_from_slice(w.reference);
        ref_off.push(refs.len() as u32);
        for reads in &w.samples {
            for (pos, cigar, b, q) in reads {
                read_pos.push(*pos);
                cigars.extend_from_slice(cigar);
                cigar_off.push(cigars.len() as u32);
                bases.extend_from_slice(b);
                quals.extend_from_slice(q);
                read_off.push(bases.len() as u32);
            }
            group_off.push(read_pos.len() as u32);
        }
    }
    let n_pos: usize = window_len.iter().map(|l| *l as usize).sum();
    let mut profile_lengths: Vec<usize> = Vec::new();
    for l in &window_len {
        let l = *l as usize;
        let step = if profile_size == 0 { l } else { profile_size };
        let mut at = 0usize;
        while at < l {
            profile_lengths.push(step.min(l - at));
            at += step;
        }
    }
    let n_profiles = profile_lengths.len();
    let mut window_status = vec![0i32; n];
    let (mut ref_depth, mut non_ref_depth) = (vec![0u32; n_pos * n_samples], vec![0u32; n_pos * n_samples]);
    let mut soft_clip_mean = vec![0f64; n_pos];
    let mut is_active_prob = vec![0f32; n_pos];
    let mut profile_prob = vec![0f32; n_pos + n_profiles * MAX_FILTER_SIZE as usize];
    let mut profile_len = vec![0u32; n_profiles];
    let mut filter_size = 0u32;
    with_engine(|h| {
        let rc = unsafe {
            phmm_activity_profile(
                h,
                n as u32,
                n_samples as u32,
                ploidy as u32,
                bq as u32,
                pseudo_counts.0,
                pseudo_counts.1,
                pseudo_counts.2,
                stand_min_conf,
                max_prob_propagation as u32,
                MAX_FILTER_SIZE,
                SIGMA,
                1,
                profile_size as u32,
                window_start.as_ptr(),
                window_len.as_ptr(),
                contig_length.as_ptr(),
                ref_off.as_ptr(),
                refs.as_ptr(),
                group_off.as_ptr(),
                read_pos.as_ptr(),
                cigar_off.as_ptr(),
                cigars.as_ptr(),
                read_off.as_ptr(),
                bases.as_ptr(),
                quals.as_ptr(),
                window_status.as_mut_ptr(),
                std::ptr::null_mut(),
                ref_depth.as_mut_ptr(),
                non_ref_depth.as_mut_ptr(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                soft_clip_mean.as_mut_ptr(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                std::ptr::null_mut(),
                is_active_prob.as_mut_ptr() as *mut std::os::raw::c_void,
                &mut filter_size,
                profile_prob.as_mut_ptr() as *mut std::os::raw::c_void,
                profile_len.as_mut_ptr(),
            )
        };
        if rc != PHMM_OK {
            panic!("HIP activity_profile failed ({}): {}", rc, last_error(h));
        }
    });
    let mut profiles = Vec::with_capacity(n_profiles);
    let mut first = 0usize;
    for (k, positions) in profile_lengths.iter().enumerate() {
        let at = first + k * MAX_FILTER_SIZE as usize;
        profiles.push(profile_prob[at..at + profile_len[k] as usize].to_vec());
        first += positions;
    }
    let depth = ref_depth.iter().zip(non_ref_depth.iter()).map(|(a, b)| a + b).collect();
    ActivityOutput { window_status, depth, soft_clip_mean, is_active_prob, profiles }
}

/// One read of `finalize_reads`: what the clip steps and the pair step read of a BAM record.  `mate` is the index inside the
/// group of the other read with the same name.
pub struct FinalizeRead<'a> {
    pub pos: i64,
    pub flags: u16,
    pub mapq: u8,
    pub mpos: i64,
    pub isize: i64,
    pub cigar: Vec<u32>,
    pub bases: &'a [u8],
    pub quals: &'a [u8],
    pub mate: Option<usize>,
}

/// One (region, sample) of `finalize_reads`: the padded span as `region.get_padded_span()` holds it, and the reads.
pub struct FinalizeGroup<'a> {
    pub span: (u64, u64),
    pub reads: Vec<FinalizeRead<'a>>,
}

/// What `finalize_reads` returns per read, in input order.  A kept read's bases are `bases[clip_first..clip_first + clip_len]`
/// of its input, its qualities the same window of `quals`; `status` is negative where the reference would panic (then `keep`
/// is false).
pub struct FinalizedRead {
    pub status: i32,
    pub keep: bool,
    pub pos: i64,
    pub unmapped: bool,
    pub clip_first: usize,
    pub clip_len: usize,
    pub cigar: Vec<u32>,
    pub unclipped_len: usize,
    pub soft_clip: (u32, u32),
    pub quals: Vec<u8>,
}

/// `AssemblyBasedCallerUtils::finalize_regions` up to its first sort with `clean_overlapping_read_pairs`
/// (src/assembly/assembly_based_caller_utils.rs:97-172, :263-289) for a batch of (region, sample) groups -- or, with `steps` =
/// `PHMM_FIN_REGION`, the map + filter of `AssemblyRegion::trim_with_padded_span` (src/assembly/assembly_region.rs:341-352).
/// The two sorts stay with the caller.
pub fn finalize_reads(groups: &[FinalizeGroup], steps: u32, min_tail_quality: u8, dont_use_soft_clipped_bases: bool) -> Vec<FinalizedRead> {
    let cfg = phmm_finalize_config {
        steps,
        min_tail_quality,
        dont_use_soft_clipped_bases: dont_use_soft_clipped_bases as u8,
        half_of_pcr_snv_qual: 20,
        reserved: 0,
    };
    let span_start: Vec<u64> = groups.iter().map(|g| g.span.0).collect();
    let span_end: Vec<u64> = groups.iter().map(|g| g.span.1).collect();
    let (mut group_off, mut cigar_off, mut read_off): (Vec<u32>, Vec<u32>, Vec<u32>) = (vec![0], vec![0], vec![0]);
    let mut out_cigar_off: Vec<u64> = vec![0];
    let (mut pos, mut mpos, mut isize_): (Vec<i64>, Vec<i64>, Vec<i64>) = (Vec::new(), Vec::new(), Vec::new());
    let mut flags: Vec<u16> = Vec::new();
    let (mut mapq, mut bases, mut quals): (Vec<u8>, Vec<u8>, Vec<u8>) = (Vec::new(), Vec::new(), Vec::new());
    let mut cigars: Vec<u32> = Vec::new();
    let mut mate: Vec<i32> = Vec::new();
    for g in groups {
        let first = pos.len();
        for r in &g.reads {
            pos.push(r.pos);
            flags.push(r.flags);
            mapq.push(r.mapq);
            mpos.push(r.mpos);
            isize_.push(r.isize);
            cigars.extend_from_slice(&r.cigar);
            cigar_off.push(cigars.len() as u32);
            out_cigar_off.push(out_cigar_off.last().unwrap() + r.cigar.len() as u64 + 2);
            bases.extend_from_slice(r.bases);
            quals.extend_from_slice(r.quals);
            read_off.push(bases.len() as u32);
            mate.push(r.mate.map(|m| (first + m) as i32).unwrap_or(-1));
        }
        group_off.push(pos.len() as u32);
    }
    let n = pos.len();
    let mut status = vec![0i32; n];
    let (mut keep, mut unmapped) = (vec![0u8; n], vec![0u8; n]);
    let mut new_pos = vec![0i64; n];
    let (mut clip_first, mut clip_len, mut n_out_cigar, mut unclipped_len) = (vec![0u32; n], vec![0u32; n], vec![0u32; n], vec![0u32; n]);
    let (mut lead_soft, mut trail_soft) = (vec![0u32; n], vec![0u32; n]);
    let mut out_cigar = vec![0u32; *out_cigar_off.last().unwrap() as usize];
    let mut out_quals = vec![0u8; quals.len()];
    with_engine(|h| {
        let rc = unsafe {
            phmm_finalize_reads(
                h,
                &cfg as *const phmm_finalize_config as *const std::os::raw::c_void,
                groups.len() as u32,
                group_off.as_ptr(),
                span_start.as_ptr(),
                span_end.as_ptr(),
                pos.as_ptr(),
                flags.as_ptr() as *const std::os::raw::c_void,
                mapq.as_ptr(),
                mpos.as_ptr(),
                isize_.as_ptr(),
                cigar_off.as_ptr(),
                cigars.as_ptr(),
                read_off.as_ptr(),
                bases.as_ptr(),
                quals.as_ptr(),
                mate.as_ptr(),
                out_cigar_off.as_ptr(),
                status.as_mut_ptr(),
                keep.as_mut_ptr(),
                new_pos.as_mut_ptr(),
                unmapped.as_mut_ptr(),
                clip_first.as_mut_ptr(),
                clip_len.as_mut_ptr(),
                out_cigar.as_mut_ptr(),
                n_out_cigar.as_mut_ptr(),
                unclipped_len.as_mut_ptr(),
                lead_soft.as_mut_ptr(),
                trail_soft.as_mut_ptr(),
                out_quals.as_mut_ptr(),
            )
        };
        if rc != PHMM_OK {
            panic!("HIP finalize_reads failed ({}): {}", rc, last_error(h));
        }
    });
    (0..n)
        .map(|r| FinalizedRead {
            status: status[r],
            keep: keep[r] != 0,
            pos: new_pos[r],
            unmapped: unmapped[r] != 0,
            clip_first: clip_first[r] as usize,
            clip_len: clip_len[r] as usize,
            cigar: out_cigar[out_cigar_off[r] as usize..out_cigar_off[r] as usize + n_out_cigar[r] as usize].to_vec(),
            unclipped_len: unclipped_len[r] as usize,
            soft_clip: (lead_soft[r], trail_soft[r]),
            quals: out_quals[read_off[r] as usize..read_off[r + 1] as usize].to_vec(),
        })
        .collect()
}

/// The arrays `phase_calls` reads, as `phmm_discover_events` (with its per-haplotype event maps), the AF step's call lists and
/// `phmm_assign_genotypes` leave them; `gt` is `[n_events][n_samples][ploidy]` indices into the call's list, -1 a no-call allele.
pub struct PhaseInput<'a> {
    pub region_event_off: &'a [u32],
    pub region_hap_off: &'a [u32],
    pub event_allele_off: &'a [u32],
    pub event_hap_allele: &'a [i32],
    pub vc_start: &'a [i64],
    pub allele_length: &'a [u32],
    pub allele_kind: &'a [u8],
    pub allele_bases_off: &'a [u32],
    pub allele_bases: &'a [u8],
    pub hap_event_off: &'a [u32],
    pub hap_event_start: &'a [i64],
    pub hap_event_alt_off: &'a [u32],
    pub hap_event_alt: &'a [u8],
    pub call_allele_off: &'a [u32],
    pub call_allele: &'a [u32],
    pub n_samples: usize,
    pub ploidy: usize,
    pub gt: &'a [i32],
}

/// What `phase_calls` returns per event, in input order.  `end` is the call's end after `reverse_trim_alleles`, the trimmed
/// allele the first `length - rev_trim` bases of each allele that is not symbolic.  `group` is `None` for an unphased call;
/// otherwise PGT is "0|1" (`phase_10 == false`) or "1|0", PS is `phase_set`, and PID is made of the start, the reference and
/// the first alt of event `leader`.  `gt` holds the sample genotypes in the order `phase_vc` leaves them.
pub struct PhasedCall {
    pub rev_trim: usize,
    pub end: i64,
    pub n_haps: usize,
    pub group: Option<usize>,
    pub phase_10: bool,
    pub leader: Option<usize>,
    pub phase_set: i64,
    pub is_phased: Vec<bool>,
    pub gt: Vec<Vec<i32>>,
}

/// The tail of `assign_genotype_likelihoods` for a batch of regions: `reverse_trim_alleles` as `make_annotated_call` applies it,
/// the called haplotypes, and `AssemblyBasedCallerUtils::phase_calls` (src/assembly/assembly_based_caller_utils.rs:975-1348).
/// Returns the calls and, per region, whether its mapping was cleared.  The strings of PGT and PID are the caller's to format.
pub fn phase_calls(input: &PhaseInput, trim: bool) -> (Vec<PhasedCall>, Vec<bool>) {
    let n_regions = if input.region_event_off.is_empty() { 0 } else { input.region_event_off.len() - 1 };
    let n_events = if n_regions > 0 { input.region_event_off[n_regions] as usize } else { 0 };
    let ns = input.n_samples;
    let pl = input.ploidy;
    let mut rev_trim = vec![0u32; n_events];
    let (mut end, mut phase_set) = (vec![0i64; n_events], vec![0i64; n_events]);
    let mut n_haps = vec![0u32; n_events];
    let (mut group, mut leader) = (vec![0i32; n_events], vec![0i32; n_events]);
    let mut phase_gt = vec![0u8; n_events];
    let (mut alt_haps, mut region_flags) = (vec![0u32; n_regions], vec![0u32; n_regions]);
    let mut is_phased = vec![0u8; n_events * ns];
    let mut gt_phased = vec![0i32; n_events * ns * pl];
    assert_eq!(input.gt.len(), n_events * ns * pl);
    with_engine(|h| {
        let rc = unsafe {
            phmm_phase_calls(
                h,
                n_regions as u32,
                input.region_event_off.as_ptr(),
                input.region_hap_off.as_ptr(),
                input.event_allele_off.as_ptr(),
                input.event_hap_allele.as_ptr(),
                input.vc_start.as_ptr(),
                input.allele_length.as_ptr(),
                input.allele_kind.as_ptr(),
                input.allele_bases_off.as_ptr(),
                input.allele_bases.as_ptr(),
                input.hap_event_off.as_ptr(),
                input.hap_event_start.as_ptr(),
                input.hap_event_alt_off.as_ptr(),
                input.hap_event_alt.as_ptr(),
                input.call_allele_off.as_ptr(),
                input.call_allele.as_ptr(),
                ns as u32,
                pl as u32,
                input.gt.as_ptr(),
                if trim { 0 } else { PHMM_PH_NO_TRIM },
                rev_trim.as_mut_ptr(),
                end.as_mut_ptr(),
                n_haps.as_mut_ptr(),
                std::ptr::null_mut(),
                group.as_mut_ptr(),
                phase_gt.as_mut_ptr(),
                leader.as_mut_ptr(),
                phase_set.as_mut_ptr(),
                alt_haps.as_mut_ptr(),
                region_flags.as_mut_ptr(),
                is_phased.as_mut_ptr(),
                gt_phased.as_mut_ptr(),
            )
        };
        if rc != PHMM_OK {
            panic!("HIP phase_calls failed ({}): {}", rc, last_error(h));
        }
    });
    let calls = (0..n_events)
        .map(|e| PhasedCall {
            rev_trim: rev_trim[e] as usize,
            end: end[e],
            n_haps: n_haps[e] as usize,
            group: if group[e] >= 0 { Some(group[e] as usize) } else { None },
            phase_10: phase_gt[e] as i32 == PHMM_PH_GT_10,
            leader: if leader[e] >= 0 { Some(leader[e] as usize) } else { None },
            phase_set: phase_set[e],
            is_phased: is_phased[e * ns..(e + 1) * ns].iter().map(|&x| x != 0).collect(),
            gt: (0..ns).map(|s| gt_phased[(e * ns + s) * pl..(e * ns + s + 1) * pl].to_vec()).collect(),
        })
        .collect();
    (calls, region_flags.iter().map(|&f| f & PHMM_PH_ABORTED != 0).collect())
}

/// One region's sequences for `assembly_kmers`: the reference haplotype and the reads with their base qualities, in the order
/// `create_graph` adds them.
pub struct AssemblyKmerRegion<'a> {
    pub reference: &'a [u8],
    pub reads: Vec<(&'a [u8], &'a [u8])>,
}

/// What `assembly_kmers` returns for one k of one region.  `ref_flags[p]` and `read_flags[r][p]` hold `PHMM_ASM_KMER_*`, a read's
/// over its bases as given (0 outside its window); `ref_ids` / `read_ids` the dense k-mer ids (`u32::MAX`: the position is not
/// scanned) a vertex map is keyed with -- empty when the call was made without ids.
pub struct AssemblyKmers {
    pub k: usize,
    pub ref_short: bool,
    pub ref_non_unique: bool,
    pub low_complexity: bool,
    pub n_sequences: usize,
    pub n_non_unique: usize,
    pub n_tracked: usize,
    pub n_distinct: usize,
    pub ref_flags: Vec<u8>,
    pub ref_ids: Vec<u32>,
    pub read_flags: Vec<Vec<u8>>,
    pub read_ids: Vec<Vec<u32>>,
}

/// The k-mer stage of `ReadThreadingAssembler::create_graph` for a batch of regions and every k in `ks` (ascending): which k are
/// rejected before a graph exists, and per position whether its k-mer is non-unique, threaded, a threading start, and its id.
/// `windows`: per read in input order (first, len) -- the read IS that part of its bases, what `finalize_reads` returns as
/// `clip_first` / `clip_len`, so no base is copied; `None`: the whole reads.  `ids`: the id planes are four fifths of the bytes
/// that come back, so a first call over every k goes without them and a second one asks for the k that survive.
/// Returns `[region][k]`.
pub fn assembly_kmers(
    regions: &[AssemblyKmerRegion],
    ks: &[usize],
    min_base_quality: u8,
    windows: Option<&[(u32, u32)]>,
    ids: bool,
) -> Vec<Vec<AssemblyKmers>> {
    let n_regions = regions.len();
    let (mut region_ref_off, mut region_read_off, mut read_off) = (vec![0u32], vec![0u32], vec![0u32]);
    let (mut ref_bases, mut read_bases, mut read_quals) = (Vec::<u8>::new(), Vec::<u8>::new(), Vec::<u8>::new());
    for g in regions {
        ref_bases.extend_from_slice(g.reference);
        region_ref_off.push(ref_bases.len() as u32);
        for (bases, quals) in g.reads.iter() {
            assert_eq!(bases.len(), quals.len());
            read_bases.extend_from_slice(bases);
            read_quals.extend_from_slice(quals);
            read_off.push(read_bases.len() as u32);
        }
        region_read_off.push((read_off.len() - 1) as u32);
    }
    let k32: Vec<u32> = ks.iter().map(|&k| k as u32).collect();
    let n_k = k32.len();
    let (n_ref, n_read) = (ref_bases.len(), read_bases.len());
    let mut flags = vec![0u32; n_k * n_regions];
    let (mut n_sequences, mut n_non_unique) = (vec![0u32; n_k * n_regions], vec![0u32; n_k * n_regions]);
    let (mut n_tracked, mut n_distinct) = (vec![0u32; n_k * n_regions], vec![0u32; n_k * n_regions]);
    let (mut ref_flags, mut read_flags) = (vec![0u8; n_k * n_ref], vec![0u8; n_k * n_read]);
    let n_ids = if ids { n_k } else { 0 };
    let (mut ref_ids, mut read_ids) = (vec![0u32; n_ids * n_ref], vec![0u32; n_ids * n_read]);
    let read_first: Vec<u32> = windows.unwrap_or(&[]).iter().map(|w| w.0).collect();
    let read_len: Vec<u32> = windows.unwrap_or(&[]).iter().map(|w| w.1).collect();
    if let Some(w) = windows {
        assert_eq!(w.len(), read_off.len() - 1);
    }
    let or_null = |v: &Vec<u32>| if windows.is_some() { v.as_ptr() } else { std::ptr::null() };
    let ids_or_null = |v: &mut Vec<u32>| if ids { v.as_mut_ptr() } else { std::ptr::null_mut() };
    with_engine(|h| {
        let rc = unsafe {
            phmm_assembly_kmers(
                h,
                n_regions as u32,
                region_ref_off.as_ptr(),
                ref_bases.as_ptr(),
                region_read_off.as_ptr(),
                read_off.as_ptr(),
                read_bases.as_ptr(),
                read_quals.as_ptr(),
                or_null(&read_first),
                or_null(&read_len),
                n_k as u32,
                k32.as_ptr(),
                min_base_quality as u32,
                flags.as_mut_ptr(),
                n_sequences.as_mut_ptr(),
                n_non_unique.as_mut_ptr(),
                n_tracked.as_mut_ptr(),
                n_distinct.as_mut_ptr(),
                ref_flags.as_mut_ptr(),
                read_flags.as_mut_ptr(),
                ids_or_null(&mut ref_ids),
                ids_or_null(&mut read_ids),
            )
        };
        if rc != PHMM_OK {
            panic!("HIP assembly_kmers failed ({}): {}", rc, last_error(h));
        }
    });
    (0..n_regions)
        .map(|g| {
            (0..n_k)
                .map(|i| {
                    let o = i * n_regions + g;
                    let (r0, r1) = (region_ref_off[g] as usize, region_ref_off[g + 1] as usize);
                    let reads = region_read_off[g] as usize..region_read_off[g + 1] as usize;
                    let span = |r: usize| i * n_read + read_off[r] as usize..i * n_read + read_off[r + 1] as usize;
                    AssemblyKmers {
                        k: ks[i],
                        ref_short: flags[o] & PHMM_ASM_REF_SHORT != 0,
                        ref_non_unique: flags[o] & PHMM_ASM_REF_NON_UNIQUE != 0,
                        low_complexity: flags[o] & PHMM_ASM_LOW_COMPLEXITY != 0,
                        n_sequences: n_sequences[o] as usize,
                        n_non_unique: n_non_unique[o] as usize,
                        n_tracked: n_tracked[o] as usize,
                        n_distinct: n_distinct[o] as usize,
                        ref_flags: ref_flags[i * n_ref + r0..i * n_ref + r1].to_vec(),
                        ref_ids: if ids { ref_ids[i * n_ref + r0..i * n_ref + r1].to_vec() } else { Vec::new() },
                        read_flags: reads.clone().map(|r| read_flags[span(r)].to_vec()).collect(),
                        read_ids: if ids { reads.clone().map(|r| read_ids[span(r)].to_vec()).collect() } else { Vec::new() },
                    }
                })
                .collect()
        })
        .collect()
}

/// One vertex of a raw read-threading graph: the occurrence that created it (`seq` 0 = the reference, 1 + r = read r of the
/// region; `pos` inside that sequence, so its bytes are `[pos, pos + k)`), whether `kmer_to_vertex_map` holds it and whether it
/// is the reference source.
pub struct AssemblyGraphVertex {
    pub seq: usize,
    pub pos: usize,
    pub tracked: bool,
    pub ref_source: bool,
}

/// One edge of a raw read-threading graph, as `MultiSampleEdge` holds it after `build_graph_if_necessary`.
pub struct AssemblyGraphEdge {
    pub source: usize,
    pub target: usize,
    pub is_ref: bool,
    pub multiplicity: usize,
    pub pruning_multiplicity: usize,
}

/// What `assembly_graph` returns for one k of one region: vertices in `NodeIndex` order, edges in `EdgeIndex` order,
/// `reference_path`, and per position of the reference and of every read (over its bases as given) the vertex it lands on,
/// `u32::MAX` where `thread_sequence` does not visit it.
pub struct AssemblyGraph {
    pub k: usize,
    pub ref_short: bool,
    pub ref_non_unique: bool,
    pub low_complexity: bool,
    pub vertices: Vec<AssemblyGraphVertex>,
    pub edges: Vec<AssemblyGraphEdge>,
    pub reference_path: Vec<u32>,
    pub ref_vertex: Vec<u32>,
    pub read_vertex: Vec<Vec<u32>>,
}

/// The raw graph `ReadThreadingAssembler::create_graph` holds right after `build_graph_if_necessary`, for a batch of regions and
/// every k in `ks` (ascending), with the default modes (dangling-branch recovery on, no counts through branches).  `samples`: a
/// sample index per read in input order, `None`: one sample; `windows` as `assembly_kmers` takes them.  Pruning, the cycle
/// checks, dangling ends and paths stay with the caller.  Returns `[region][k]`.
pub fn assembly_graph(
    regions: &[AssemblyKmerRegion],
    ks: &[usize],
    min_base_quality: u8,
    windows: Option<&[(u32, u32)]>,
    samples: Option<&[u32]>,
    num_pruning_samples: usize,
) -> Vec<Vec<AssemblyGraph>> {
    let n_regions = regions.len();
    let (mut region_ref_off, mut region_read_off, mut read_off) = (vec![0u32], vec![0u32], vec![0u32]);
    let (mut ref_bases, mut read_bases, mut read_quals) = (Vec::<u8>::new(), Vec::<u8>::new(), Vec::<u8>::new());
    for g in regions {
        ref_bases.extend_from_slice(g.reference);
        region_ref_off.push(ref_bases.len() as u32);
        for (bases, quals) in g.reads.iter() {
            assert_eq!(bases.len(), quals.len());
            read_bases.extend_from_slice(bases);
            read_quals.extend_from_slice(quals);
            read_off.push(read_bases.len() as u32);
        }
        region_read_off.push((read_off.len() - 1) as u32);
    }
    let k32: Vec<u32> = ks.iter().map(|&k| k as u32).collect();
    let n_k = k32.len();
    let n_graphs = n_k * n_regions;
    let (n_ref, n_read) = (ref_bases.len(), read_bases.len());
    let read_first: Vec<u32> = windows.unwrap_or(&[]).iter().map(|w| w.0).collect();
    let read_len: Vec<u32> = windows.unwrap_or(&[]).iter().map(|w| w.1).collect();
    if let Some(w) = windows {
        assert_eq!(w.len(), read_off.len() - 1);
    }
    if let Some(s) = samples {
        assert_eq!(s.len(), read_off.len() - 1);
    }
    let or_null = |v: &Vec<u32>| if windows.is_some() { v.as_ptr() } else { std::ptr::null() };
    let (mut flags, mut n_vertices, mut n_edges, mut n_ref_path) =
        (vec![0u32; n_graphs], vec![0u32; n_graphs], vec![0u32; n_graphs], vec![0u32; n_graphs]);
    let (mut vertex_off, mut edge_off, mut ref_path_off) = (vec![0u32; n_graphs + 1], vec![0u32; n_graphs + 1], vec![0u32; n_graphs + 1]);
    let (mut ref_vertex, mut read_vertex) = (vec![u32::MAX; n_k * n_ref], vec![u32::MAX; n_k * n_read]);
    let (mut vertex_seq, mut vertex_pos, mut vertex_flags) = (Vec::<u32>::new(), Vec::<u32>::new(), Vec::<u8>::new());
    let (mut edge_src, mut edge_dst, mut edge_is_ref) = (Vec::<u32>::new(), Vec::<u32>::new(), Vec::<u8>::new());
    let (mut edge_multiplicity, mut edge_pruning, mut ref_path) = (Vec::<u32>::new(), Vec::<u32>::new(), Vec::<u32>::new());
    let mut capacity = [0u32; 3];
    let mut required = [0u32; 3];
    with_engine(|h| {
        for pass in 0..2 {
            let rc = unsafe {
                phmm_assembly_graph(
                    h,
                    n_regions as u32,
                    region_ref_off.as_ptr(),
                    ref_bases.as_ptr(),
                    region_read_off.as_ptr(),
                    read_off.as_ptr(),
                    read_bases.as_ptr(),
                    read_quals.as_ptr(),
                    or_null(&read_first),
                    or_null(&read_len),
                    if let Some(s) = samples { s.as_ptr() } else { std::ptr::null() },
                    n_k as u32,
                    k32.as_ptr(),
                    min_base_quality as u32,
                    num_pruning_samples as u32,
                    capacity.as_ptr(),
                    required.as_mut_ptr(),
                    flags.as_mut_ptr(),
                    n_vertices.as_mut_ptr(),
                    n_edges.as_mut_ptr(),
                    n_ref_path.as_mut_ptr(),
                    vertex_off.as_mut_ptr(),
                    edge_off.as_mut_ptr(),
                    ref_path_off.as_mut_ptr(),
                    vertex_seq.as_mut_ptr(),
                    vertex_pos.as_mut_ptr(),
                    vertex_flags.as_mut_ptr(),
                    edge_src.as_mut_ptr(),
                    edge_dst.as_mut_ptr(),
                    edge_is_ref.as_mut_ptr(),
                    edge_multiplicity.as_mut_ptr(),
                    edge_pruning.as_mut_ptr(),
                    ref_path.as_mut_ptr(),
                    ref_vertex.as_mut_ptr(),
                    read_vertex.as_mut_ptr(),
                )
            };
            if rc == PHMM_ERR_EVENT_CAPACITY && pass == 0 {
                capacity = required;
                let (nv, ne, np) = (required[0] as usize, required[1] as usize, required[2] as usize);
                vertex_seq = vec![0u32; nv];
                vertex_pos = vec![0u32; nv];
                vertex_flags = vec![0u8; nv];
                edge_src = vec![0u32; ne];
                edge_dst = vec![0u32; ne];
                edge_is_ref = vec![0u8; ne];
                edge_multiplicity = vec![0u32; ne];
                edge_pruning = vec![0u32; ne];
                ref_path = vec![0u32; np];
                continue;
            }
            if rc != PHMM_OK {
                panic!("HIP assembly_graph failed ({}): {}", rc, last_error(h));
            }
            break;
        }
    });
    (0..n_regions)
        .map(|g| {
            (0..n_k)
                .map(|i| {
                    let o = i * n_regions + g;
                    let (r0, r1) = (region_ref_off[g] as usize, region_ref_off[g + 1] as usize);
                    let reads = region_read_off[g] as usize..region_read_off[g + 1] as usize;
                    let span = |r: usize| i * n_read + read_off[r] as usize..i * n_read + read_off[r + 1] as usize;
                    let vertices = vertex_off[o] as usize..vertex_off[o + 1] as usize;
                    let edges = edge_off[o] as usize..edge_off[o + 1] as usize;
                    AssemblyGraph {
                        k: ks[i],
                        ref_short: flags[o] & PHMM_ASM_REF_SHORT != 0,
                        ref_non_unique: flags[o] & PHMM_ASM_REF_NON_UNIQUE != 0,
                        low_complexity: flags[o] & PHMM_ASM_LOW_COMPLEXITY != 0,
                        vertices: vertices
                            .map(|v| AssemblyGraphVertex {
                                seq: vertex_seq[v] as usize,
                                pos: vertex_pos[v] as usize,
                                tracked: vertex_flags[v] as u32 & PHMM_GRAPH_VERTEX_TRACKED != 0,
                                ref_source: vertex_flags[v] as u32 & PHMM_GRAPH_VERTEX_REF_SOURCE != 0,
                            })
                            .collect(),
                        edges: edges
                            .map(|e| AssemblyGraphEdge {
                                source: edge_src[e] as usize,
                                target: edge_dst[e] as usize,
                                is_ref: edge_is_ref[e] != 0,
                                multiplicity: edge_multiplicity[e] as usize,
                                pruning_multiplicity: edge_pruning[e] as usize,
                            })
                            .collect(),
                        reference_path: ref_path[ref_path_off[o] as usize..ref_path_off[o + 1] as usize].to_vec(),
                        ref_vertex: ref_vertex[i * n_ref + r0..i * n_ref + r1].to_vec(),
                        read_vertex: reads.map(|r| read_vertex[span(r)].to_vec()).collect(),
                    }
                })
                .collect()
        })
        .collect()
}

/// What `assembly_prune` returns for one graph.  `edge_chain[e]` is the `EdgeIndex` of the head of the chain `find_all_chains`
/// puts edge `e` in, `u32::MAX` for an edge in no chain; `edge_state` and `vertex_state` hold `PHMM_PRUNE_*` bits.
pub struct PrunedGraph {
    pub has_cycle: bool,
    pub no_ref_ends: bool,
    pub n_chains: usize,
    pub n_chains_removed: usize,
    pub n_vertices_left: usize,
    pub n_edges_left: usize,
    pub ref_source: Option<usize>,
    pub ref_sink: Option<usize>,
    pub edge_chain: Vec<u32>,
    pub edge_state: Vec<u8>,
    pub vertex_state: Vec<u8>,
}

/// What `create_graph` does to the raw graphs of `assembly_graph` before it looks for paths: `prune_low_weight_chains` with the
/// low-weight pruner and one factor per graph (`PHMM_PRUNE_OP_CHAINS`), `has_cycles`, the reference ends, the vertices
/// dangling-end recovery starts from, and `remove_paths_not_connected_to_ref` (`PHMM_PRUNE_OP_CONNECT`).  `absent`: per graph
/// the vertices and the edges that are vacant slots by now, `None`: none are.  The adaptive pruner, dangling-end recovery
/// itself and paths stay with the caller.
pub fn assembly_prune(
    graphs: &[&AssemblyGraph],
    prune_factors: &[usize],
    ops: u32,
    absent: Option<&[(Vec<u8>, Vec<u8>)]>,
) -> Vec<PrunedGraph> {
    let n_graphs = graphs.len();
    assert_eq!(prune_factors.len(), n_graphs);
    let (mut vertex_off, mut edge_off) = (vec![0u32], vec![0u32]);
    let (mut edge_src, mut edge_dst, mut edge_is_ref, mut edge_pruning) = (Vec::<u32>::new(), Vec::<u32>::new(), Vec::<u8>::new(), Vec::<u32>::new());
    let (mut vertex_absent, mut edge_absent) = (Vec::<u8>::new(), Vec::<u8>::new());
    for (i, g) in graphs.iter().enumerate() {
        for e in g.edges.iter() {
            edge_src.push(e.source as u32);
            edge_dst.push(e.target as u32);
            edge_is_ref.push(e.is_ref as u8);
            edge_pruning.push(e.pruning_multiplicity as u32);
        }
        if let Some(a) = absent {
            assert_eq!((a[i].0.len(), a[i].1.len()), (g.vertices.len(), g.edges.len()));
            vertex_absent.extend_from_slice(&a[i].0);
            edge_absent.extend_from_slice(&a[i].1);
        }
        vertex_off.push(vertex_off[i] + g.vertices.len() as u32);
        edge_off.push(edge_src.len() as u32);
    }
    let factor: Vec<u32> = prune_factors.iter().map(|&f| f.min(u32::MAX as usize) as u32).collect();
    let (n_v, n_e) = (vertex_off[n_graphs] as usize, edge_src.len());
    let or_null = |v: &Vec<u8>| if absent.is_some() { v.as_ptr() } else { std::ptr::null() };
    let (mut graph_flags, mut n_chains, mut n_chains_removed) = (vec![0u32; n_graphs], vec![0u32; n_graphs], vec![0u32; n_graphs]);
    let (mut n_vertices_left, mut n_edges_left) = (vec![0u32; n_graphs], vec![0u32; n_graphs]);
    let (mut ref_source, mut ref_sink) = (vec![u32::MAX; n_graphs], vec![u32::MAX; n_graphs]);
    let (mut edge_chain, mut edge_state, mut vertex_state) = (vec![u32::MAX; n_e], vec![0u8; n_e], vec![0u8; n_v]);
    with_engine(|h| {
        let rc = unsafe {
            phmm_assembly_prune(
                h,
                n_graphs as u32,
                vertex_off.as_ptr(),
                edge_off.as_ptr(),
                edge_src.as_ptr(),
                edge_dst.as_ptr(),
                edge_is_ref.as_ptr(),
                edge_pruning.as_ptr(),
                or_null(&vertex_absent),
                or_null(&edge_absent),
                ops,
                factor.as_ptr(),
                graph_flags.as_mut_ptr(),
                n_chains.as_mut_ptr(),
                n_chains_removed.as_mut_ptr(),
                n_vertices_left.as_mut_ptr(),
                n_edges_left.as_mut_ptr(),
                ref_source.as_mut_ptr(),
                ref_sink.as_mut_ptr(),
                edge_chain.as_mut_ptr(),
                edge_state.as_mut_ptr(),
                vertex_state.as_mut_ptr(),
            )
        };
        if rc != PHMM_OK {
            panic!("HIP assembly_prune failed ({}): {}", rc, last_error(h));
        }
    });
    let index = |v: u32| if v == u32::MAX { None } else { Some(v as usize) };
    (0..n_graphs)
        .map(|o| {
            let vertices = vertex_off[o] as usize..vertex_off[o + 1] as usize;
            let edges = edge_off[o] as usize..edge_off[o + 1] as usize;
            PrunedGraph {
                has_cycle: graph_flags[o] & PHMM_PRUNE_HAS_CYCLE != 0,
                no_ref_ends: graph_flags[o] & PHMM_PRUNE_NO_REF_ENDS != 0,
                n_chains: n_chains[o] as usize,
                n_chains_removed: n_chains_removed[o] as usize,
                n_vertices_left: n_vertices_left[o] as usize,
                n_edges_left: n_edges_left[o] as usize,
                ref_source: index(ref_source[o]),
                ref_sink: index(ref_sink[o]),
                edge_chain: edge_chain[edges.clone()].to_vec(),
                edge_state: edge_state[edges].to_vec(),
                vertex_state: vertex_state[vertices].to_vec(),
            }
        })
        .collect()
}

/// What `assembly_recover` returns: the arrays of `phmm_assembly_recover` as the header lays them out, cut to what was written.
pub struct RecoveredEnds {
    pub per_graph: Vec<[u32; 7]>,
    pub end_off: Vec<u32>,
    pub new_edge_off: Vec<u32>,
    pub new_vertex_off: Vec<u32>,
    pub end_vertex: Vec<u32>,
    pub end_kind: Vec<u32>,
    pub end_status: Vec<u32>,
    pub end_alt_len: Vec<u32>,
    pub end_ref_len: Vec<u32>,
    pub end_n_cigar: Vec<u32>,
    pub end_cigar: Vec<u32>,
    pub end_edge: Vec<u32>,
    pub new_edge_src: Vec<u32>,
    pub new_edge_dst: Vec<u32>,
    pub new_edge_multiplicity: Vec<u32>,
    pub new_edge_pruning_multiplicity: Vec<u32>,
    pub new_vertex_kmer: Vec<u8>,
    pub edge_removed: Vec<u8>,
}

/// The dense arrays `assembly_recover` reads: the regions as `assembly_graph` packed them and the graphs as it returned them,
/// k-major, with the masks `assembly_prune` left (empty slices: no element is absent).
pub struct RecoverInput<'a> {
    pub region_ref_off: &'a [u32],
    pub ref_bases: &'a [u8],
    pub region_read_off: &'a [u32],
    pub read_off: &'a [u32],
    pub read_bases: &'a [u8],
    pub k: &'a [u32],
    pub vertex_off: &'a [u32],
    pub edge_off: &'a [u32],
    pub vertex_seq: &'a [u32],
    pub vertex_pos: &'a [u32],
    pub edge_src: &'a [u32],
    pub edge_dst: &'a [u32],
    pub edge_is_ref: &'a [u8],
    pub edge_multiplicity: &'a [u32],
    pub edge_pruning_multiplicity: &'a [u32],
    pub vertex_absent: &'a [u8],
    pub edge_absent: &'a [u8],
    pub prune_factor: &'a [u32],
}

/// Dangling-end recovery for many graphs: `recover_dangling_tails`, then `recover_dangling_heads`, with
/// `recover_all_dangling_branches = false`.  Asks for the sizes first (capacities 0), then calls again with them.  Not compiled
/// here and bound to no call site: the assembler's `get_assembly_result` still recovers on the host.
pub fn assembly_recover(input: &RecoverInput, cfg: &phmm_recover_config) -> RecoveredEnds {
    let n_regions = input.region_ref_off.len().max(1) - 1;
    let n_graphs = input.k.len() * n_regions;
    let k_max = input.k.iter().copied().max().unwrap_or(0) as usize;
    let masks = !input.vertex_absent.is_empty() || !input.edge_absent.is_empty();
    let or_null = |v: &[u8]| if masks { v.as_ptr() } else { std::ptr::null() };
    let mut capacity = [0u32; 3];
    let mut required = [0u32; 3];
    loop {
        let mut per = vec![vec![0u32; n_graphs]; 7];
        let (mut end_off, mut new_edge_off, mut new_vertex_off) = (vec![0u32; n_graphs + 1], vec![0u32; n_graphs + 1], vec![0u32; n_graphs + 1]);
        let mut ends = vec![vec![0u32; capacity[0] as usize]; 7];
        let mut end_cigar = vec![0u32; 4 * capacity[0] as usize];
        let mut edges = vec![vec![0u32; capacity[1] as usize]; 4];
        let mut new_vertex_kmer = vec![0u8; capacity[2] as usize * k_max];
        let mut edge_removed = vec![0u8; input.edge_src.len()];
        let mut rc = PHMM_OK;
        with_engine(|h| {
            rc = unsafe {
                phmm_assembly_recover(
                    h,
                    cfg as *const phmm_recover_config as *const std::os::raw::c_void,
                    n_regions as u32,
                    input.region_ref_off.as_ptr(),
                    input.ref_bases.as_ptr(),
                    input.region_read_off.as_ptr(),
                    input.read_off.as_ptr(),
                    input.read_bases.as_ptr(),
                    std::ptr::null(),
                    std::ptr::null(),
                    input.k.len() as u32,
                    input.k.as_ptr(),
                    input.vertex_off.as_ptr(),
                    input.edge_off.as_ptr(),
                    input.vertex_seq.as_ptr(),
                    input.vertex_pos.as_ptr(),
                    input.edge_src.as_ptr(),
                    input.edge_dst.as_ptr(),
                    input.edge_is_ref.as_ptr(),
                    input.edge_multiplicity.as_ptr(),
                    input.edge_pruning_multiplicity.as_ptr(),
                    or_null(input.vertex_absent),
                    or_null(input.edge_absent),
                    std::ptr::null(),
                    input.prune_factor.as_ptr(),
                    capacity.as_ptr(),
                    required.as_mut_ptr(),
                    per[0].as_mut_ptr(),
                    per[1].as_mut_ptr(),
                    per[2].as_mut_ptr(),
                    per[3].as_mut_ptr(),
                    per[4].as_mut_ptr(),
                    per[5].as_mut_ptr(),
                    per[6].as_mut_ptr(),
                    end_off.as_mut_ptr(),
                    new_edge_off.as_mut_ptr(),
                    new_vertex_off.as_mut_ptr(),
                    ends[0].as_mut_ptr(),
                    ends[1].as_mut_ptr(),
                    ends[2].as_mut_ptr(),
                    ends[3].as_mut_ptr(),
                    ends[4].as_mut_ptr(),
                    ends[5].as_mut_ptr(),
                    end_cigar.as_mut_ptr(),
                    ends[6].as_mut_ptr(),
                    edges[0].as_mut_ptr(),
                    edges[1].as_mut_ptr(),
                    edges[2].as_mut_ptr(),
                    edges[3].as_mut_ptr(),
                    new_vertex_kmer.as_mut_ptr(),
                    edge_removed.as_mut_ptr(),
                )
            };
            if rc != PHMM_OK && rc != PHMM_ERR_EVENT_CAPACITY {
                panic!("HIP assembly_recover failed ({}): {}", rc, last_error(h));
            }
        });
        if rc == PHMM_ERR_EVENT_CAPACITY {
            capacity = required;
            continue;
        }
        let mut edges = edges.into_iter();
        let mut ends = ends.into_iter();
        let mut next_end = || ends.next().unwrap();
        let (end_vertex, end_kind, end_status, end_alt_len, end_ref_len, end_n_cigar, end_edge) =
            (next_end(), next_end(), next_end(), next_end(), next_end(), next_end(), next_end());
        return RecoveredEnds {
            per_graph: (0..n_graphs).map(|g| [per[0][g], per[1][g], per[2][g], per[3][g], per[4][g], per[5][g], per[6][g]]).collect(),
            end_off,
            new_edge_off,
            new_vertex_off,
            end_vertex,
            end_kind,
            end_status,
            end_alt_len,
            end_ref_len,
            end_n_cigar,
            end_cigar,
            end_edge,
            new_edge_src: edges.next().unwrap(),
            new_edge_dst: edges.next().unwrap(),
            new_edge_multiplicity: edges.next().unwrap(),
            new_edge_pruning_multiplicity: edges.next().unwrap(),
            new_vertex_kmer,
            edge_removed,
        };
    }
}

/// What `assembly_seqgraph` returns: the arrays of `phmm_assembly_seqgraph` as the header lays them out, cut to what was written.
/// `per_graph`: status, sequence vertices, edges, bytes, chains zipped, edges cleaned, vertices unconnected, reference source, sink.
pub struct SequenceGraphs {
    pub per_graph: Vec<[u32; 9]>,
    pub seq_vertex_off: Vec<u32>,
    pub seq_edge_off: Vec<u32>,
    pub seq_base_off: Vec<u32>,
    pub seq_vertex_base_off: Vec<u32>,
    pub seq_vertex_first: Vec<u32>,
    pub seq_vertex_n_merged: Vec<u32>,
    pub seq_edge_src: Vec<u32>,
    pub seq_edge_dst: Vec<u32>,
    pub seq_edge_is_ref: Vec<u8>,
    pub seq_edge_multiplicity: Vec<u32>,
    pub seq_bases: Vec<u8>,
    pub vertex_to_seq: Vec<u32>,
}

/// The dense arrays `assembly_seqgraph` reads: the regions as `assembly_graph` packed them, the raw vertices' `vertex_seq` /
/// `vertex_pos`, and the graphs as recovery and `assembly_prune(CONNECT)` left them, k-major (empty slices: no new vertices, no
/// absent element, no flags).
pub struct SequenceGraphInput<'a> {
    pub region_ref_off: &'a [u32],
    pub ref_bases: &'a [u8],
    pub region_read_off: &'a [u32],
    pub read_off: &'a [u32],
    pub read_bases: &'a [u8],
    pub k: &'a [u32],
    pub vertex_off: &'a [u32],
    pub edge_off: &'a [u32],
    pub vertex_seq: &'a [u32],
    pub vertex_pos: &'a [u32],
    pub edge_src: &'a [u32],
    pub edge_dst: &'a [u32],
    pub edge_is_ref: &'a [u8],
    pub edge_multiplicity: &'a [u32],
    pub new_vertex_off: &'a [u32],
    pub new_vertex_kmer: &'a [u8],
    pub vertex_absent: &'a [u8],
    pub edge_absent: &'a [u8],
    pub graph_flags: &'a [u32],
}

/// The zipped sequence graph of many graphs: `to_sequence_graph`, `clean_non_ref_paths`, the first `zip_linear_chains`, the
/// orphans and `remove_vertices_not_connected_to_ref_regardless_of_edge_direction`.  Asks for the sizes first (capacities 0), then
/// calls again with them.  Not compiled here and bound to no call site: the assembler's `get_assembly_result` still builds its
/// sequence graph on the host.
pub fn assembly_seqgraph(input: &SequenceGraphInput) -> SequenceGraphs {
    let n_regions = input.region_ref_off.len().max(1) - 1;
    let n_graphs = input.k.len() * n_regions;
    let masks = !input.vertex_absent.is_empty() || !input.edge_absent.is_empty();
    let or_null = |v: &[u8]| if masks { v.as_ptr() } else { std::ptr::null() };
    let news = !input.new_vertex_off.is_empty();
    let mut capacity = [0u32; 3];
    let mut required = [0u32; 3];
    loop {
        let mut per = vec![vec![0u32; n_graphs]; 9];
        let mut offs = vec![vec![0u32; n_graphs + 1]; 3];
        let mut vertices = vec![vec![0u32; capacity[0] as usize]; 3];
        let mut edges = vec![vec![0u32; capacity[1] as usize]; 3];
        let mut seq_edge_is_ref = vec![0u8; capacity[1] as usize];
        let mut seq_bases = vec![0u8; capacity[2] as usize];
        let mut vertex_to_seq = vec![0u32; input.vertex_off.last().copied().unwrap_or(0) as usize];
        let mut rc = PHMM_OK;
        with_engine(|h| {
            rc = unsafe {
                phmm_assembly_seqgraph(
                    h,
                    n_regions as u32,
                    input.region_ref_off.as_ptr(),
                    input.ref_bases.as_ptr(),
                    input.region_read_off.as_ptr(),
                    input.read_off.as_ptr(),
                    input.read_bases.as_ptr(),
                    std::ptr::null(),
                    std::ptr::null(),
                    input.k.len() as u32,
                    input.k.as_ptr(),
                    input.vertex_off.as_ptr(),
                    input.edge_off.as_ptr(),
                    input.vertex_seq.as_ptr(),
                    input.vertex_pos.as_ptr(),
                    input.edge_src.as_ptr(),
                    input.edge_dst.as_ptr(),
                    input.edge_is_ref.as_ptr(),
                    input.edge_multiplicity.as_ptr(),
                    if news { input.new_vertex_off.as_ptr() } else { std::ptr::null() },
                    if news { input.new_vertex_kmer.as_ptr() } else { std::ptr::null() },
                    or_null(input.vertex_absent),
                    or_null(input.edge_absent),
                    if input.graph_flags.is_empty() { std::ptr::null() } else { input.graph_flags.as_ptr() },
                    capacity.as_ptr(),
                    required.as_mut_ptr(),
                    per[0].as_mut_ptr(),
                    per[1].as_mut_ptr(),
                    per[2].as_mut_ptr(),
                    per[3].as_mut_ptr(),
                    per[4].as_mut_ptr(),
                    per[5].as_mut_ptr(),
                    per[6].as_mut_ptr(),
                    per[7].as_mut_ptr(),
                    per[8].as_mut_ptr(),
                    offs[0].as_mut_ptr(),
                    offs[1].as_mut_ptr(),
                    offs[2].as_mut_ptr(),
                    vertices[0].as_mut_ptr(),
                    vertices[1].as_mut_ptr(),
                    vertices[2].as_mut_ptr(),
                    edges[0].as_mut_ptr(),
                    edges[1].as_mut_ptr(),
                    seq_edge_is_ref.as_mut_ptr(),
                    edges[2].as_mut_ptr(),
                    seq_bases.as_mut_ptr(),
                    vertex_to_seq.as_mut_ptr(),
                )
            };
            if rc != PHMM_OK && rc != PHMM_ERR_EVENT_CAPACITY {
                panic!("HIP assembly_seqgraph failed ({}): {}", rc, last_error(h));
            }
        });
        if rc == PHMM_ERR_EVENT_CAPACITY {
            capacity = required;
            continue;
        }
        let mut offs = offs.into_iter();
        let mut vertices = vertices.into_iter();
        let mut edges = edges.into_iter();
        return SequenceGraphs {
            per_graph: (0..n_graphs).map(|g| [per[0][g], per[1][g], per[2][g], per[3][g], per[4][g], per[5][g], per[6][g], per[7][g], per[8][g]]).collect(),
            seq_vertex_off: offs.next().unwrap(),
            seq_edge_off: offs.next().unwrap(),
            seq_base_off: offs.next().unwrap(),
            seq_vertex_base_off: vertices.next().unwrap(),
            seq_vertex_first: vertices.next().unwrap(),
            seq_vertex_n_merged: vertices.next().unwrap(),
            seq_edge_src: edges.next().unwrap(),
            seq_edge_dst: edges.next().unwrap(),
            seq_edge_is_ref,
            seq_edge_multiplicity: edges.next().unwrap(),
            seq_bases,
            vertex_to_seq,
        };
    }
}

/// What `assembly_best_paths` returns: the arrays of `phmm_assembly_best_paths` as the header lays them out, cut to what was
/// written.  `per_graph`: status (`PHMM_PATHS_*`), paths, queue pops, edges and vertices the cycle removal took.  `hap_off` /
/// `hap_bases` are the `alt_off` / `alt_bases` of `calculate_cigar`.
pub struct BestPaths {
    pub per_graph: Vec<[u32; 5]>,
    pub path_off: Vec<u32>,
    pub path_edge_off: Vec<u32>,
    pub hap_base_off: Vec<u32>,
    pub path_score: Vec<f64>,
    pub path_is_ref: Vec<u8>,
    pub path_n_edges: Vec<u32>,
    pub hap_off: Vec<u32>,
    pub path_first_equal: Vec<u32>,
    pub path_edges: Vec<u32>,
    pub hap_bases: Vec<u8>,
}

/// The k best haplotype paths of the graphs `assembly_seqgraph` returned, k-major: `GraphBasedKBestHaplotypeFinder` from each
/// graph's reference source to its reference sink, `Path::get_bases`, and which paths `find_best_path` would find in its result
/// set already (`regions`: `n_k` graphs per region, `region_ref_off` and `ref_bases` of the regions' reference haplotypes; `None`
/// asks for no duplicate marks and leaves `path_first_equal` empty).  Asks for the sizes first (capacities 0), then calls again
/// with them: two passes at the most.  Not compiled here and bound to no call site: `find_best_path` still searches on the host.
pub fn assembly_best_paths(
    graphs: &SequenceGraphs,
    regions: Option<(usize, &[u32], &[u8])>,
    max_paths: u32,
    max_nodes_per_graph: u32,
) -> BestPaths {
    let n_graphs = graphs.per_graph.len();
    let (n_k, n_regions) = match regions {
        Some((n_k, region_ref_off, _)) => (n_k, region_ref_off.len().max(1) - 1),
        None => (0, 0),
    };
    let (region_ref_off, ref_bases) = match regions {
        Some((_, region_ref_off, ref_bases)) => (region_ref_off.as_ptr(), ref_bases.as_ptr()),
        None => (std::ptr::null(), std::ptr::null()),
    };
    let status: Vec<u32> = graphs.per_graph.iter().map(|g| g[0]).collect();
    let source: Vec<u32> = graphs.per_graph.iter().map(|g| g[7]).collect();
    let sink: Vec<u32> = graphs.per_graph.iter().map(|g| g[8]).collect();
    let mut capacity = [0u32; 3];
    let mut required = [0u32; 3];
    for pass in 0..2 {
        let mut per = vec![vec![0u32; n_graphs]; 5];
        let mut offs = vec![vec![0u32; n_graphs + 1]; 3];
        let mut path_score = vec![0f64; capacity[0] as usize];
        let mut path_is_ref = vec![0u8; capacity[0] as usize];
        let mut path_n_edges = vec![0u32; capacity[0] as usize];
        let mut hap_off = vec![0u32; capacity[0] as usize + 1];
        let mut path_first_equal = vec![0u32; if regions.is_some() { capacity[0] as usize } else { 0 }];
        let mut path_edges = vec![0u32; capacity[1] as usize];
        let mut hap_bases = vec![0u8; capacity[2] as usize];
        let mut rc = PHMM_OK;
        with_engine(|h| {
            rc = unsafe {
                phmm_assembly_best_paths(
                    h,
                    n_graphs as u32,
                    graphs.seq_vertex_off.as_ptr(),
                    graphs.seq_edge_off.as_ptr(),
                    graphs.seq_base_off.as_ptr(),
                    graphs.seq_vertex_base_off.as_ptr(),
                    graphs.seq_edge_src.as_ptr(),
                    graphs.seq_edge_dst.as_ptr(),
                    graphs.seq_edge_is_ref.as_ptr(),
                    graphs.seq_edge_multiplicity.as_ptr(),
                    graphs.seq_bases.as_ptr(),
                    status.as_ptr(),
                    source.as_ptr(),
                    sink.as_ptr(),
                    std::ptr::null(),
                    max_paths,
                    max_nodes_per_graph,
                    n_regions as u32,
                    n_k as u32,
                    region_ref_off,
                    ref_bases,
                    capacity.as_ptr(),
                    required.as_mut_ptr(),
                    per[0].as_mut_ptr(),
                    per[1].as_mut_ptr(),
                    per[2].as_mut_ptr(),
                    per[3].as_mut_ptr(),
                    per[4].as_mut_ptr(),
                    offs[0].as_mut_ptr(),
                    offs[1].as_mut_ptr(),
                    offs[2].as_mut_ptr(),
                    path_score.as_mut_ptr(),
                    path_is_ref.as_mut_ptr(),
                    path_n_edges.as_mut_ptr(),
                    hap_off.as_mut_ptr(),
                    if regions.is_some() { path_first_equal.as_mut_ptr() } else { std::ptr::null_mut() },
                    path_edges.as_mut_ptr(),
                    hap_bases.as_mut_ptr(),
                    std::ptr::null_mut(),
                    std::ptr::null_mut(),
                )
            };
            if rc != PHMM_OK && rc != PHMM_ERR_EVENT_CAPACITY {
                panic!("HIP assembly_best_paths failed ({}): {}", rc, last_error(h));
            }
        });
        if rc == PHMM_ERR_EVENT_CAPACITY {
            if pass == 1 {
                panic!("HIP assembly_best_paths: the sizes {:?} it asked for did not suffice", capacity);
            }
            capacity = required;
            continue;
        }
        let mut offs = offs.into_iter();
        return BestPaths {
            per_graph: (0..n_graphs).map(|g| [per[0][g], per[1][g], per[2][g], per[3][g], per[4][g]]).collect(),
            path_off: offs.next().unwrap(),
            path_edge_off: offs.next().unwrap(),
            hap_base_off: offs.next().unwrap(),
            path_score,
            path_is_ref,
            path_n_edges,
            hap_off,
            path_first_equal,
            path_edges,
            hap_bases,
        };
    }
    unreachable!("the second pass returns or panics")
}

/// One haplotype of the assembler's result set for `trim_regions`: its bases, CIGAR, `alignment_start_hap_wrt_ref`, genome
/// location (closed) and whether it is the reference haplotype.
pub struct TrimHaplotype<'a> {
    pub bases: &'a [u8],
    pub cigar: &'a [rust_htslib::bam::record::Cigar],
    pub start_wrt_ref: usize,
    pub loc: (usize, usize),
    pub is_ref: bool,
}

/// One region for `trim_regions`: `full_reference_with_padding` and where it starts, the active span and the padded span (closed),
/// the haplotypes in the set's insertion order.
pub struct TrimRegion<'a> {
    pub reference: &'a [u8],
    pub ref_start: usize,
    pub active: (usize, usize),
    pub padded: (usize, usize),
    pub haplotypes: Vec<TrimHaplotype<'a>>,
}

/// A trimmed haplotype as `trim_to` leaves it; `source` is its index among the region's input haplotypes.
pub struct TrimmedHaplotype {
    pub bases: Vec<u8>,
    pub cigar: rust_htslib::bam::record::CigarString,
    pub start_wrt_ref: usize,
    pub is_ref: bool,
    pub source: usize,
}

/// What `trim_regions` returns for one region.  `status` < 0: the reference returns the empty model (`PHMM_EV_STATUS_*`) or
/// panics (`PHMM_TRIM_STATUS_*`) there.  `span_variation` is the trimmer's `is_variation_present`, `set_variation` the result
/// set's `variation_present` after `trim_to`; `fates[i]` is the rank of input haplotype i or a `PHMM_TRIM_FATE_*`.
pub struct TrimmedRegion {
    pub status: i32,
    pub span_variation: bool,
    pub set_variation: bool,
    pub variant_span: (usize, usize),
    pub padded_span: (usize, usize),
    pub new_active: (usize, usize),
    pub new_padded: (usize, usize),
    pub fates: Vec<i32>,
    pub dup_of: Vec<Option<usize>>,
    pub haplotypes: Vec<TrimmedHaplotype>,
    pub ref_haplotype: Option<usize>,
}

/// `get_variation_events`, `AssemblyRegionTrimmer::trim` (legacy trimming off) and `AssemblyResultSet::trim_to` of
/// `call_region` (haplotype_caller_engine.rs:1194-1243) for a batch of regions.  `padding`: SNP, indel and STR padding and
/// `max_extension_into_region_padding` in THIS order (`AssemblyRegionTrimmer::new` takes the indel padding first).
pub fn trim_regions(regions: &[TrimRegion], max_mnp_distance: usize, padding: [usize; 4]) -> Vec<TrimmedRegion> {
    let n_regions = regions.len();
    let (mut region_ref_off, mut region_hap_off, mut hap_off, mut hap_cigar_off) = (vec![0u32], vec![0u32], vec![0u32], vec![0u32]);
    let (mut ref_bases, mut hap_bases, mut hap_cigar) = (Vec::<u8>::new(), Vec::<u8>::new(), Vec::<u32>::new());
    let (mut ref_start, mut active_start, mut active_end) = (Vec::<u64>::new(), Vec::<u64>::new(), Vec::<u64>::new());
    let (mut padded_start, mut padded_end) = (Vec::<u64>::new(), Vec::<u64>::new());
    let (mut hap_start, mut loc_start, mut loc_end, mut is_ref) = (Vec::<u32>::new(), Vec::<u64>::new(), Vec::<u64>::new(), Vec::<u8>::new());
    for g in regions {
        ref_bases.extend_from_slice(g.reference);
        region_ref_off.push(ref_bases.len() as u32);
        ref_start.push(g.ref_start as u64);
        active_start.push(g.active.0 as u64);
        active_end.push(g.active.1 as u64);
        padded_start.push(g.padded.0 as u64);
        padded_end.push(g.padded.1 as u64);
        for hap in g.haplotypes.iter() {
            hap_bases.extend_from_slice(hap.bases);
            hap_off.push(hap_bases.len() as u32);
            hap_cigar.extend_from_slice(&encode_cigar(hap.cigar));
            hap_cigar_off.push(hap_cigar.len() as u32);
            hap_start.push(hap.start_wrt_ref as u32);
            loc_start.push(hap.loc.0 as u64);
            loc_end.push(hap.loc.1 as u64);
            is_ref.push(hap.is_ref as u8);
        }
        region_hap_off.push(hap_start.len() as u32);
    }
    let n_haps = hap_start.len();
    let pad: Vec<u32> = padding.iter().map(|&p| p as u32).collect();
    let mut status = vec![0i32; n_regions];
    let mut variation = vec![0u8; n_regions];
    let mut spans = vec![vec![0u64; n_regions]; 8];
    let (mut fate, mut dup_of) = (vec![0i32; n_haps], vec![0u32; n_haps]);
    let (mut out_region_hap_off, mut out_hap_off, mut out_cigar_off) = (vec![0u32; n_regions + 1], vec![0u32; n_haps + 1], vec![0u32; n_haps + 1]);
    let (mut out_bases, mut out_cigar) = (vec![0u8; hap_bases.len()], vec![0u32; hap_cigar.len()]);
    let (mut out_start, mut out_source, mut out_is_ref) = (vec![0u32; n_haps], vec![0u32; n_haps], vec![0u8; n_haps]);
    let mut ref_hap = vec![0i32; n_regions];
    let span_ptr: Vec<*mut u64> = spans.iter_mut().map(|v| v.as_mut_ptr()).collect();
    with_engine(|h| {
        let rc = unsafe {
            phmm_trim_regions(
                h,
                n_regions as u32,
                region_ref_off.as_ptr(),
                ref_bases.as_ptr(),
                ref_start.as_ptr(),
                active_start.as_ptr(),
                active_end.as_ptr(),
                padded_start.as_ptr(),
                padded_end.as_ptr(),
                region_hap_off.as_ptr(),
                hap_off.as_ptr(),
                hap_bases.as_ptr(),
                hap_cigar_off.as_ptr(),
                hap_cigar.as_ptr(),
                hap_start.as_ptr(),
                loc_start.as_ptr(),
                loc_end.as_ptr(),
                is_ref.as_ptr(),
                max_mnp_distance as u32,
                pad.as_ptr(),
                status.as_mut_ptr(),
                variation.as_mut_ptr(),
                span_ptr[0],
                span_ptr[1],
                span_ptr[2],
                span_ptr[3],
                span_ptr[4],
                span_ptr[5],
                span_ptr[6],
                span_ptr[7],
                fate.as_mut_ptr(),
                dup_of.as_mut_ptr(),
                out_region_hap_off.as_mut_ptr(),
                out_hap_off.as_mut_ptr(),
                out_bases.as_mut_ptr(),
                out_cigar_off.as_mut_ptr(),
                out_cigar.as_mut_ptr(),
                out_start.as_mut_ptr(),
                out_source.as_mut_ptr(),
                out_is_ref.as_mut_ptr(),
                ref_hap.as_mut_ptr(),
            )
        };
        if rc != PHMM_OK {
            panic!("HIP trim_regions failed ({}): {}", rc, last_error(h));
        }
    });
    let pair = |k: usize, g: usize| (spans[k][g] as usize, spans[k + 1][g] as usize);
    (0..n_regions)
        .map(|g| {
            let haps = region_hap_off[g] as usize..region_hap_off[g + 1] as usize;
            let outs = out_region_hap_off[g] as usize..out_region_hap_off[g + 1] as usize;
            TrimmedRegion {
                status: status[g],
                span_variation: variation[g] as u32 & PHMM_TRIM_VARIATION_SPAN != 0,
                set_variation: variation[g] as u32 & PHMM_TRIM_VARIATION_SET != 0,
                variant_span: pair(0, g),
                padded_span: pair(2, g),
                new_active: pair(4, g),
                new_padded: pair(6, g),
                fates: fate[haps.clone()].to_vec(),
                dup_of: dup_of[haps].iter().map(|&d| if d == u32::MAX { None } else { Some(d as usize) }).collect(),
                haplotypes: outs
                    .map(|k| TrimmedHaplotype {
                        bases: out_bases[out_hap_off[k] as usize..out_hap_off[k + 1] as usize].to_vec(),
                        cigar: decode_cigar(&out_cigar[out_cigar_off[k] as usize..out_cigar_off[k + 1] as usize]),
                        start_wrt_ref: out_start[k] as usize,
                        is_ref: out_is_ref[k] != 0,
                        source: out_source[k] as usize,
                    })
                    .collect(),
                ref_haplotype: if ref_hap[g] < 0 { None } else { Some(ref_hap[g] as usize) },
            }
        })
        .collect()
}

/// One activity profile for `assembly_regions`: its band-passed state list (`is_active_prob` per state), the position of state 0,
/// the position of the last state that was ADDED (`region_stop_loc`), the contig's length, and the window whose staged reads
/// are its reads.
pub struct RegionProfile<'a> {
    pub probs: &'a [f32],
    pub start: usize,
    pub stop: usize,
    pub contig_length: usize,
    pub window: usize,
}

/// The staged reads of `assembly_regions`, as `activity_profile` takes them: per (window, sample) group, window-major, the
/// reads in fetch order with `pos` not decreasing.
pub struct RegionReads<'a> {
    pub n_windows: usize,
    pub n_samples: usize,
    pub group_read_off: &'a [u32],
    pub read_pos: &'a [i64],
    pub read_cigar_off: &'a [u32],
    pub read_cigar: &'a [u32],
    pub read_off: &'a [u32],
    pub read_quals: &'a [u8],
}

/// One assembly region as `pop_ready_assembly_regions` returns it (closed spans), with what `fill_next_assembly_region_with_reads`
/// decides before its sorts: `reads[sample]` are global indices of the staged reads in input order.
pub struct DeviceAssemblyRegion {
    pub active_span: (usize, usize),
    pub padded_span: (usize, usize),
    pub n_states: usize,
    pub is_active: bool,
    pub forced: bool,
    pub over_depth: bool,
    pub activity_density: f32,
    pub reads: Vec<Vec<u32>>,
}

/// What `assembly_regions` returns: per profile its status (`PHMM_REG_STATUS_*` where the reference panics) and its regions;
/// per staged read the depth cap's key, `sum(qual as f64) / len as f64`.
pub struct DeviceAssemblyRegions {
    pub status: Vec<i32>,
    pub regions: Vec<Vec<DeviceAssemblyRegion>>,
    pub read_mean_qual: Vec<f64>,
}

/// `ActivityProfile::pop_ready_assembly_regions` (activity_profile.rs:371-668) for a batch of profiles and, with `reads`, the
/// staged reads a fetch of each region's padded span returns (assembly_region_iterator.rs:54-159 without BAM I/O and
/// `read_is_filtered`).  The depth cap's sort and `take`, and the final sort by `BirdToolRead::cmp`, stay with the caller.
pub fn assembly_regions(
    profiles: &[RegionProfile],
    reads: Option<&RegionReads>,
    assembly_region_extension: usize,
    min_region_size: usize,
    max_region_size: usize,
    max_prob_propagation: usize,
    active_prob_threshold: f32,
    max_input_depth: usize,
) -> DeviceAssemblyRegions {
    let n_profiles = profiles.len();
    let mut prob = Vec::<f32>::new();
    let (mut first, mut len, mut window) = (Vec::<u32>::new(), Vec::<u32>::new(), Vec::<u32>::new());
    let (mut start, mut stop, mut contig) = (Vec::<u64>::new(), Vec::<u64>::new(), Vec::<u64>::new());
    for p in profiles {
        first.push(prob.len() as u32);
        len.push(p.probs.len() as u32);
        prob.extend_from_slice(p.probs);
        start.push(p.start as u64);
        stop.push(p.stop as u64);
        contig.push(p.contig_length as u64);
        window.push(p.window as u32);
    }
    let null32 = std::ptr::null::<u32>();
    let (n_windows, n_samples, n_reads) = match reads {
        Some(r) => (r.n_windows, r.n_samples, r.read_pos.len()),
        None => (0, 0, 0),
    };
    // without reads the six arrays are NULL and the call skips part B
    let (group_read_off, read_pos, read_cigar_off, read_cigar, read_base_off, read_quals) = match reads {
        Some(r) => (r.group_read_off.as_ptr(), r.read_pos.as_ptr(), r.read_cigar_off.as_ptr(), r.read_cigar.as_ptr(), r.read_off.as_ptr(), r.read_quals.as_ptr()),
        None => (null32, std::ptr::null::<i64>(), null32, null32, null32, std::ptr::null::<u8>()),
    };
    let mut status = vec![0i32; n_profiles];
    let mut region_off = vec![0u32; n_profiles + 1];
    let mut mean_qual = vec![0f64; n_reads];
    let mut required = [0u32; 2];
    let mut capacity = [0u32; 2];
    let (mut spans, mut words) = (vec![Vec::<u64>::new(); 4], vec![Vec::<u32>::new(); 3]);
    let (mut density, mut read_off, mut members) = (Vec::<f32>::new(), Vec::<u32>::new(), Vec::<u32>::new());
    with_engine(|h| {
        // the first call asks for the sizes (all capacities 0), the second fills arrays of exactly those sizes
        for pass in 0..2 {
            let (r, m) = (capacity[0] as usize, capacity[1] as usize);
            spans = vec![vec![0u64; r]; 4];
            words = vec![vec![0u32; r]; 3];
            density = vec![0f32; r];
            read_off = vec![0u32; r * n_samples.max(1) + 1];
            members = vec![0u32; m];
            let rc = unsafe {
                phmm_assembly_regions(
                    h,
                    n_profiles as u32,
                    n_windows as u32,
                    n_samples as u32,
                    assembly_region_extension as u32,
                    min_region_size as u32,
                    max_region_size as u32,
                    max_prob_propagation as u32,
                    active_prob_threshold as f64,
                    max_input_depth.min(u32::MAX as usize) as u32,
                    prob.len() as u32,
                    prob.as_ptr() as *const std::os::raw::c_void,
                    first.as_ptr(),
                    len.as_ptr(),
                    start.as_ptr(),
                    stop.as_ptr(),
                    contig.as_ptr(),
                    window.as_ptr(),
                    group_read_off,
                    read_pos,
                    read_cigar_off,
                    read_cigar,
                    read_base_off,
                    read_quals,
                    capacity.as_ptr(),
                    required.as_mut_ptr(),
                    status.as_mut_ptr(),
                    region_off.as_mut_ptr(),
                    spans[0].as_mut_ptr(),
                    spans[1].as_mut_ptr(),
                    spans[2].as_mut_ptr(),
                    spans[3].as_mut_ptr(),
                    words[0].as_mut_ptr(),
                    words[1].as_mut_ptr(),
                    density.as_mut_ptr() as *mut std::os::raw::c_void,
                    words[2].as_mut_ptr(),
                    read_off.as_mut_ptr(),
                    members.as_mut_ptr(),
                    mean_qual.as_mut_ptr(),
                )
            };
            if rc == PHMM_ERR_EVENT_CAPACITY && pass == 0 {
                capacity = required;
                continue;
            }
            if rc != PHMM_OK {
                panic!("HIP assembly_regions failed ({}): {}", rc, last_error(h));
            }
            break;
        }
    });
    let regions = (0..n_profiles)
        .map(|k| {
            (region_off[k] as usize..region_off[k + 1] as usize)
                .map(|r| DeviceAssemblyRegion {
                    active_span: (spans[0][r] as usize, spans[1][r] as usize),
                    padded_span: (spans[2][r] as usize, spans[3][r] as usize),
                    n_states: words[0][r] as usize,
                    is_active: words[1][r] & PHMM_REG_ACTIVE != 0,
                    forced: words[1][r] & PHMM_REG_FORCED != 0,
                    over_depth: words[1][r] & PHMM_REG_OVER_DEPTH != 0,
                    activity_density: density[r],
                    reads: (0..n_samples)   // (0 without reads)
                        .map(|s| members[read_off[r * n_samples + s] as usize..read_off[r * n_samples + s + 1] as usize].to_vec())
                        .collect(),
                })
                .collect()
        })
        .collect();
    DeviceAssemblyRegions { status, regions, read_mean_qual: mean_qual }
}
