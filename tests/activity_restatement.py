"""Test infrastructure, not product code: a statement-by-statement restatement of the reference's activity profile, what
tests/test_activity_hip.py holds phmm_activity_profile to.

  parse_record, alignment_context_creation, next_to_soft_clip, is_alt, next_to_soft_clip_or_indel,
  check_position_against_cigar, count_high_quality_soft_clips, update_heterozygous_likelihood, update_ref_vs_any_results
                         src/haplotype/haplotype_caller_engine.rs:738-899, :1464-1749 -- the reference's own loops, `continue`
                         and `break` where they stand (the I element's `continue` skips `cig_index += 1`)
  RunningAverage         src/utils/math_utils.rs:434-477 (mean only: nothing reads s)
  qual_to_prob_log10, qual_to_error_prob_log10, qual_to_prob     src/utils/quality_utils.rs:37-44, :82-104
  make_kernel, determine_filter_size, normal_distribution, normalize_sum_to_one
                         src/activity_profile/band_pass_activity_profile.rs:36-105, math_utils.rs:383-415
  ActivityProfile / BandPassActivityProfile: add, process_state, incorporate_single_state, get_loc_for_offset
                         src/activity_profile/activity_profile.rs:193-341, band_pass_activity_profile.rs:210-280 -- the
                         incremental scatter on a growing list, NOT a gather: the device gathers, so the comparison means something
  the per-position loop of calculate_activity_probabilities      haplotype_caller_engine.rs:1012-1107

PLs come from genotype_restatement.gls_to_pls, the allele-frequency step from af_restatement.calculate_genotypes (alleles: the
reference and one symbolic allele of length 0).  Floats are Python's (f64, the platform libm) and numpy.float32 scalars where
the reference computes in f32.

`trace`, where given, counts how often each quirk was met (tests/test_activity_oracle.py's census)."""
import functools
import math
from collections import Counter

import numpy as np

import af_restatement as AF
import genotype_restatement as G

REF_MODEL_DELETION_QUAL = 30                 # haplotype_caller_engine.rs:111
HQ_BASE_QUALITY_SOFTCLIP_THRESHOLD = 28      # :117
AVERAGE_HQ_SOFTCLIPS_HQ_BASES_THRESHOLD = 6.0  # :75
MIN_PROB_TO_KEEP_IN_FILTER = 1e-5            # band_pass_activity_profile.rs:25
MAX_FILTER_SIZE, DEFAULT_SIGMA = 50, 17.0    # :24, :26
ROOT_TWO_PI = math.sqrt(2.0 * math.pi)       # math_utils.rs:22
REF_SKIP, CIGAR_OVERRUN = -1, -2             # PHMM_ACT_STATUS_*
OPS = "MIDNSHP=X"
F32 = np.float32


class ReferencePanic(Exception):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


def parse_cigar(cigar):
    """A CIGAR string, [(op, length)] with op a letter or a BAM code, or BAM-encoded integers -> [(letter, length)]."""
    if isinstance(cigar, str):
        out, n = [], ""
        for ch in cigar:
            if ch.isdigit():
                n += ch
            else:
                out.append((ch, int(n)))
                n = ""
        return out
    out = []
    for c in cigar:
        if isinstance(c, (tuple, list)):
            out.append((c[0] if isinstance(c[0], str) else OPS[c[0]], int(c[1])))
        else:
            out.append((OPS[int(c) & 15], int(c) >> 4))
    return out


class Record:
    def __init__(self, pos, cigar, seq, qual):
        self.pos, self.cigar, self.seq, self.qual = int(pos), parse_cigar(cigar), bytes(seq), [int(q) for q in qual]


class RunningAverage:
    def __init__(self):
        self.mean_, self.obs_count = 0.0, 0

    def add(self, obs):
        self.obs_count += 1
        self.mean_ += (obs - self.mean_) / float(self.obs_count)

    def mean(self):
        return self.mean_


class RefVsAnyResult:
    def __init__(self, likelihoodcount):
        self.genotype_likelihoods = [0.0] * likelihoodcount
        self.read_counts = self.ref_depth = self.non_ref_depth = 0


def cigar_consumes_read_bases(op):
    return op in "MIS=X"


def qual_to_prob_log10(qual):
    x = 1.0 - 10.0 ** (float(qual) / -10.0)
    return math.log10(x) if x > 0.0 else -math.inf


def qual_to_error_prob_log10(qual):
    return float(qual) * -0.1


@functools.lru_cache(maxsize=None)
def approximate_log10_sum_log10(a, b):
    """math_utils.rs:314-332 through genotype_restatement's (memoised: the same few (quality, genotype) pairs come back)."""
    return float(G.approximate_log10_sum_log10(np.array([a]), np.array([b]))[0])


def check_position_against_cigar(op, check_indels):
    next_to_soft_clip = False
    if op == "S":
        next_to_soft_clip = True
    elif op in "ID":
        if check_indels:
            next_to_soft_clip = True
    return next_to_soft_clip


def next_to_soft_clip_or_indel(record, qpos, check_indels, trace=None):
    read_cursor = 0
    end_of_cigar_read_cursor = 0
    next_to_soft_clip = False
    qpos_to_cigar_cursor = qpos + 1
    for op, n in record.cigar:
        if cigar_consumes_read_bases(op):
            end_of_cigar_read_cursor = read_cursor + n
        if qpos_to_cigar_cursor == read_cursor:
            next_to_soft_clip = check_position_against_cigar(op, check_indels)
        elif qpos_to_cigar_cursor - 1 == end_of_cigar_read_cursor:
            next_to_soft_clip = check_position_against_cigar(op, check_indels)
            if trace is not None:
                trace["else_if_arm"] += 1
        past_query_pos = read_cursor >= qpos
        if past_query_pos or next_to_soft_clip:
            if trace is not None and past_query_pos and not next_to_soft_clip:
                trace["break_on_past_query_pos"] += 1
            break
        if cigar_consumes_read_bases(op):
            read_cursor += n
    return next_to_soft_clip


def next_to_soft_clip(record, cig_index, qpos, trace=None):
    if qpos is not None:
        return next_to_soft_clip_or_indel(record, qpos, False, trace)
    c = record.cigar
    return (c[max(cig_index - 1, 0)][0] == "S" or c[min(cig_index + 1, len(c) - 1)][0] == "S" or c[cig_index][0] == "S")


def is_alt(record, qpos, refr_base, trace=None):
    if qpos is not None:
        read_char = record.seq[qpos]
        next_to_sc_indel = next_to_soft_clip_or_indel(record, qpos, True, trace)
        return bytes([read_char]).upper() != bytes([refr_base]).upper() or next_to_sc_indel
    return True


def count_high_quality_soft_clips(record, min_soft_clip_qual):
    num_high_quality_soft_clips = 0.0
    align_pos = 0
    for op, n in record.cigar:
        if op == "S":
            for _ in range(n):
                qual_pos = record.qual[align_pos]
                align_pos += 1
                if qual_pos > min_soft_clip_qual:
                    num_high_quality_soft_clips += 1.0
        elif cigar_consumes_read_bases(op):
            align_pos += n
    return num_high_quality_soft_clips


def update_heterozygous_likelihood(result, likelihoodcount, log10ploidy, ref_likelihood, non_ref_likelihood):
    gl = result.genotype_likelihoods
    gl[0] += ref_likelihood + log10ploidy
    gl[likelihoodcount - 1] += non_ref_likelihood + log10ploidy
    i, j = 1, likelihoodcount - 2
    while i < likelihoodcount - 1:
        gl[i] += approximate_log10_sum_log10(ref_likelihood + math.log10(float(j)), non_ref_likelihood + math.log10(float(i)))
        i += 1
        j -= 1


def alignment_context_creation(qpos, is_del, record, result, hq_soft_clips, log10ploidy, likelihoodcount, refr_base, bq, cig_index,
                               trace=None):
    record_qual = REF_MODEL_DELETION_QUAL if is_del else record.qual[qpos]
    alt = False
    if record_qual >= bq or is_del:
        result.read_counts += 1
        alt = is_alt(record, qpos, refr_base, trace)
        if alt:
            result.non_ref_depth += 1
            non_ref_likelihood = qual_to_prob_log10(record_qual)
            ref_likelihood = qual_to_error_prob_log10(record_qual) + (-(math.log10(3.0)))
        else:
            result.ref_depth += 1
            ref_likelihood = qual_to_prob_log10(record_qual)
            non_ref_likelihood = qual_to_error_prob_log10(record_qual) + (-(math.log10(3.0)))
        update_heterozygous_likelihood(result, likelihoodcount, log10ploidy, ref_likelihood, non_ref_likelihood)
    elif trace is not None:
        trace["uncounted_base"] += 1
    if alt and next_to_soft_clip(record, cig_index, qpos, trace):
        hq_soft_clips.add(count_high_quality_soft_clips(record, HQ_BASE_QUALITY_SOFTCLIP_THRESHOLD))
        if trace is not None:
            trace["soft_clips_added"] += 1


def parse_record(record, positions, subtractor, bq, likelihoodcount, sequence_at, log10ploidy, bound_start, bound_end, trace=None):
    """positions: [(RunningAverage, RefVsAnyResult)] of the window; sequence_at(pos): reference_reader.current_sequence[pos]."""
    read_cursor = 0
    pos = record.pos
    cig_index = 0
    true_index = 0  # (not the reference's: where cig_index would stand without the skipped increment, for the census)
    touched = Counter()
    for op, n in record.cigar:
        true_index += 1
        if op == "D":
            for _ in range(n):
                if pos < bound_start:
                    pos += 1
                    continue
                elif pos >= bound_end:
                    if trace is not None:
                        trace["del_past_bound_end"] += 1
                    break
                if trace is not None and cig_index != true_index - 1:
                    trace["deletion_with_lagging_cig_index"] += 1
                    c = record.cigar
                    t = true_index - 1
                    if next_to_soft_clip(record, cig_index, None) != (c[max(t - 1, 0)][0] == "S" or c[min(t + 1, len(c) - 1)][0] == "S"):
                        trace["lagging_cig_index_changes_the_answer"] += 1
                hq_soft_clips, result = positions[max(pos - subtractor, 0)]
                alignment_context_creation(None, True, record, result, hq_soft_clips, log10ploidy, likelihoodcount, sequence_at(pos), bq,
                                           cig_index, trace)
                touched[pos] += 1
                pos += 1
        elif op == "N":
            raise ReferencePanic(REF_SKIP)
        elif op == "I":
            if pos < bound_start:
                read_cursor += n
                if trace is not None:
                    trace["ins_before_bound_start"] += 1
                continue
            elif pos >= bound_end:
                if trace is not None:
                    trace["ins_past_bound_end"] += 1
                break
            if read_cursor >= len(record.qual):
                raise ReferencePanic(CIGAR_OVERRUN)
            hq_soft_clips, result = positions[max(pos - subtractor, 0)]
            alignment_context_creation(read_cursor, False, record, result, hq_soft_clips, log10ploidy, likelihoodcount, sequence_at(pos),
                                       bq, cig_index, trace)
            touched[pos] += 1
            if trace is not None:
                trace["ins_entry"] += 1
            read_cursor += n
        elif op in "XM=":
            for _ in range(n):
                if pos < bound_start:
                    read_cursor += 1
                    pos += 1
                    continue
                elif pos >= bound_end:
                    if trace is not None:
                        trace["match_past_bound_end"] += 1
                    break
                if read_cursor >= len(record.qual):
                    raise ReferencePanic(CIGAR_OVERRUN)
                hq_soft_clips, result = positions[max(pos - subtractor, 0)]
                alignment_context_creation(read_cursor, False, record, result, hq_soft_clips, log10ploidy, likelihoodcount,
                                           sequence_at(pos), bq, cig_index, trace)
                touched[pos] += 1
                read_cursor += 1
                pos += 1
        elif op == "S":
            read_cursor += n
        cig_index += 1
    if trace is not None:
        trace["two_slots_of_one_read_at_one_position"] += sum(1 for v in touched.values() if v > 1)
        if record.pos < bound_start and touched:
            trace["read_crosses_window_start"] += 1
        if touched and pos >= bound_end:
            trace["read_crosses_window_end"] += 1


def contract_status(reads):
    """What phmm_activity_profile reports for a window: the panics above, for every read of the window whether or not the
    reference's loop reaches the element (its contract is a superset of the reference's panics)."""
    for r in reads:
        if any(op == "N" for op, _ in r.cigar):
            return REF_SKIP
        if sum(n for op, n in r.cigar if cigar_consumes_read_bases(op)) > len(r.qual):
            return CIGAR_OVERRUN
    return 0


def update_activity_profile(samples, ref, window_start, window_len, target_len, ploidy, bq, trace=None):
    """update_activity_profile for every sample of one window -> (per sample [RefVsAnyResult], [RunningAverage]).  samples: per
    sample its Records in fetch order; ref: the reference bases from window_start on."""
    likelihoodcount = ploidy + 1
    log10ploidy = math.log10(float(ploidy))
    per_contig_per_base_hq_soft_clips = [RunningAverage() for _ in range(window_len)]
    current_likelihoods = []
    for reads in samples:
        likelihoods = [RefVsAnyResult(likelihoodcount) for _ in range(window_len)]
        positions = list(zip(per_contig_per_base_hq_soft_clips, likelihoods))
        for record in reads:
            parse_record(record, positions, min(window_start, target_len), bq, likelihoodcount, lambda pos: ref[pos - window_start],
                         log10ploidy, window_start, min(window_start + window_len, target_len), trace)
        for result in likelihoods:  # update_ref_vs_any_results
            denominator = float(result.read_counts) * log10ploidy
            for i in range(likelihoodcount):
                result.genotype_likelihoods[i] -= denominator
        current_likelihoods.append(likelihoods)
    return current_likelihoods, per_contig_per_base_hq_soft_clips


# ---- the band-pass ------------------------------------------------------------------------------------------------------------

def normal_distribution(mean, sd, x):
    assert sd >= 0.0
    return math.exp(-(x - mean) * (x - mean) / (2.0 * sd * sd)) / (sd * ROOT_TWO_PI)


def normalize_sum_to_one(array):
    if not array:
        return array
    s = 0.0
    for x in array:
        s += x
    assert s >= 0.0
    return [x / s for x in array]


def make_kernel(filter_size, sigma):
    return normalize_sum_to_one([normal_distribution(float(filter_size), sigma, float(i)) for i in range(2 * filter_size + 1)])


def determine_filter_size(kernel, min_prob_to_keep_in_filter):
    middle = (len(kernel) - 1) // 2
    filter_end = middle
    while filter_end > 0:
        if kernel[filter_end - 1] < min_prob_to_keep_in_filter:
            break
        filter_end -= 1
    return middle - filter_end


class ActivityProfile:
    """The state list holds active_prob (numpy.float32) per position from region_start_loc; a state's result type is kept
    beside it only while it is processed."""

    def __init__(self, max_prob_propagation_distance, contig_len):
        self.max_prob_propagation_distance = max_prob_propagation_distance
        self.contig_len = contig_len
        self.state_list = []
        self.region_start_loc = self.region_stop_loc = None

    def get_loc_for_offset(self, relative_loc, offset):
        start = relative_loc + offset
        if start < 0 or start > self.contig_len:
            return None
        return start

    def process_state(self, loc, prob, hq_clips):
        """hq_clips: None, or the f32 value of HighQualitySoftClips."""
        if hq_clips is not None:
            states = []
            num_hq_clips = int(min(hq_clips, F32(self.max_prob_propagation_distance)))
            for i in range(-num_hq_clips, num_hq_clips + 1):
                at = self.get_loc_for_offset(loc, i)
                if at is not None:
                    states.append((at, prob))
            return states
        return [(loc, prob)]

    def incorporate_single_state(self, at, prob):
        position = at - self.region_start_loc
        assert position <= len(self.state_list), "Must add state contiguous to existing states"
        if position >= 0:
            if position < len(self.state_list):
                self.state_list[position] = self.state_list[position] + prob
            else:
                self.state_list.append(prob)

    def add(self, loc, prob, hq_clips):
        if not self.state_list:
            self.region_start_loc = self.region_stop_loc = loc
        else:
            assert self.region_stop_loc == loc - 1, "Bad add call to ActivityProfile"
            self.region_stop_loc = loc
        for at, p in self.process_state(loc, prob, hq_clips):
            self.incorporate_single_state(at, p)


class BandPassActivityProfile(ActivityProfile):
    def __init__(self, max_prob_propagation_distance, max_filter_size, sigma, adaptive_filter_size, contig_len):
        super().__init__(max_prob_propagation_distance, contig_len)
        full_kernel = make_kernel(max_filter_size, sigma)
        self.filter_size = determine_filter_size(full_kernel, MIN_PROB_TO_KEEP_IN_FILTER) if adaptive_filter_size else max_filter_size
        self.gaussian_kernel = make_kernel(self.filter_size, sigma)

    def super_process_state(self, loc, prob, hq_clips):
        return ActivityProfile.process_state(self, loc, prob, hq_clips)

    def process_state(self, loc, prob, hq_clips):
        states = []
        for _, super_prob in self.super_process_state(loc, prob, hq_clips):
            if super_prob > 0.0:
                for i in range(-self.filter_size, self.filter_size + 1):
                    at = self.get_loc_for_offset(loc, i)
                    if at is not None:
                        states.append((at, super_prob * F32(self.gaussian_kernel[i + self.filter_size])))
            else:
                states.append((loc, prob))
        return states

def band_pass(states, contig_len, max_prob_propagation=50, max_filter_size=MAX_FILTER_SIZE, sigma=DEFAULT_SIGMA, adaptive=True):
    """states: [(loc, prob, soft-clip mean or None)] contiguous -> the profile's state list as float32."""
    prof = BandPassActivityProfile(max_prob_propagation, max_filter_size, sigma, adaptive, contig_len)
    for loc, prob, clips in states:
        hq = None
        if clips is not None and F32(clips) >= F32(AVERAGE_HQ_SOFTCLIPS_HQ_BASES_THRESHOLD):  # ActivityProfileDataType::new
            hq = F32(clips)
        prof.add(loc, F32(prob), hq)
    return np.array(prof.state_list, np.float32), prof


# ---- the whole stage --------------------------------------------------------------------------------------------------------

def saturating_u8(x):
    """Rust's `f64 as u8`."""
    if x != x or x <= 0.0:
        return 0
    return 255 if x >= 255.0 else int(x)


def qual_to_prob(qual):
    return 1.0 - 10.0 ** (float(qual) / -10.0)


_AF_CACHE = {}


def is_active(pls, ploidy, pseudo, stand_min_conf):
    """calculate_genotypes on the fake alleles for one position: (qual, flags, margin, is_active_prob as float32).  Memoised: it is
    a pure function of its arguments."""
    key = (tuple(tuple(int(x) for x in p) for p in pls), ploidy, tuple(pseudo), stand_min_conf)
    if key not in _AF_CACHE:
        r = AF.calculate_genotypes([(ploidy, list(p)) for p in key[0]], [1, 0], [AF.PLAIN, AF.PLAIN], pseudo, stand_min_conf)
        called = bool(r["flags"] & AF.CALLED)
        prob = F32(qual_to_prob(saturating_u8(r["qual"]))) if called else F32(0.0)
        _AF_CACHE[key] = (r["qual"], r["flags"], r["margin"], prob)
    return _AF_CACHE[key]


def activity_profile(windows, ploidy=2, min_base_quality=10, pseudo_counts=(10.0, 0.01, 0.00125), stand_min_conf=0.0,
                     max_prob_propagation=50, max_filter_size=MAX_FILTER_SIZE, sigma=DEFAULT_SIGMA, adaptive_filter_size=True,
                     profile_size=0, trace=None):
    """windows: [(start, ref bytes, contig_length, per sample [(pos, cigar, bases, quals)])] -> a dict of numpy arrays in the layout
    of phmm_activity_profile (lorikeet_amd.activity.ActivityResult), `profiles` (the state lists, one array per profile) and
    `mult` (how many states each position's state turned into)."""
    n_samples = len(windows[0][3]) if windows else 1
    G1 = ploidy + 1
    P = sum(len(w[1]) for w in windows)
    out = dict(window_status=np.zeros(len(windows), np.int32), read_counts=np.zeros((P, n_samples), np.uint32),
               ref_depth=np.zeros((P, n_samples), np.uint32), non_ref_depth=np.zeros((P, n_samples), np.uint32),
               gl=np.zeros((P, n_samples, G1)), pl=np.zeros((P, n_samples, G1), np.int32), soft_clip_mean=np.zeros(P),
               soft_clip_count=np.zeros(P, np.uint32), qual=np.zeros(P), af_flags=np.zeros(P, np.uint32),
               is_active_prob=np.zeros(P, np.float32), margin=np.full(P, np.inf), mult=np.ones(P, np.int64), profiles=[],
               profile_window=[], profile_start=[])
    base = 0
    for w, (start, ref, contig_len, samples) in enumerate(windows):
        n = len(ref)
        records = [[Record(*r) for r in reads] for reads in samples]
        status = contract_status([r for reads in records for r in reads])
        step = profile_size or n
        if status == 0:
            try:
                likelihoods, clips = update_activity_profile(records, ref, start, n, contig_len, ploidy, min_base_quality, trace)
            except ReferencePanic as e:  # (contract_status names every one of them first)
                status = e.status
        out["window_status"][w] = status
        for at in range(0, n, step or 1):
            m = min(step, n - at)
            out["profile_window"].append(w)
            out["profile_start"].append(start + at)
            if status != 0:
                out["profiles"].append(np.zeros(0, np.float32))
                continue
            prof = BandPassActivityProfile(max_prob_propagation, max_filter_size, sigma, adaptive_filter_size, contig_len)
            for pos in range(at, at + m):
                g = base + pos
                pls = []
                for s in range(n_samples):
                    r = likelihoods[s][pos]
                    out["read_counts"][g, s], out["ref_depth"][g, s], out["non_ref_depth"][g, s] = r.read_counts, r.ref_depth, r.non_ref_depth
                    out["gl"][g, s] = r.genotype_likelihoods
                    out["pl"][g, s] = G.gls_to_pls(np.array(r.genotype_likelihoods))
                    pls.append(out["pl"][g, s])
                out["soft_clip_mean"][g], out["soft_clip_count"][g] = clips[pos].mean(), clips[pos].obs_count
                out["qual"][g], out["af_flags"][g], out["margin"][g], prob = is_active(pls, ploidy, pseudo_counts, stand_min_conf)
                out["is_active_prob"][g] = prob
                mean32 = F32(clips[pos].mean())
                hq = mean32 if mean32 >= F32(AVERAGE_HQ_SOFTCLIPS_HQ_BASES_THRESHOLD) else None
                out["mult"][g] = len(prof.super_process_state(start + pos, prob, hq))
                prof.add(start + pos, prob, hq)
            out["profiles"].append(np.array(prof.state_list, np.float32))
        base += n
    probe = BandPassActivityProfile(max_prob_propagation, max_filter_size, sigma, adaptive_filter_size, 0)
    out["filter_size"] = probe.filter_size
    out["kernel"] = probe.gaussian_kernel
    return out


def term_table(ploidy):
    """What update_heterozygous_likelihood adds for (is_alt, quality): [2][256][ploidy + 1], through the functions above."""
    t = np.zeros((2, 256, ploidy + 1))
    log10ploidy = math.log10(float(ploidy))
    for alt in (0, 1):
        for q in range(256):
            r = RefVsAnyResult(ploidy + 1)
            right, wrong = qual_to_prob_log10(q), qual_to_error_prob_log10(q) + (-(math.log10(3.0)))
            update_heterozygous_likelihood(r, ploidy + 1, log10ploidy, wrong if alt else right, right if alt else wrong)
            t[alt, q] = r.genotype_likelihoods
    return t
