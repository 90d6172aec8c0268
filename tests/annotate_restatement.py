"""Test infrastructure, not product code: a statement-by-statement restatement of what the reference does with the read
likelihoods of a called event, what tests/test_annotate_hip.py holds phmm_annotate_events to (integers exact, doubles bit
for bit).

  the call's marginal   haplotype_caller_genotyping_engine.rs:376-384 (the one-to-one subset) with
                        AlleleLikelihoods::marginalize (src/model/allele_likelihoods.rs:633-740), after retain_evidence's
                        overlap predicate (genotype_restatement.overlaps / marginalize)
  search_best_allele    allele_likelihoods.rs:457-554 with can_be_reference = true, as best_alleles_tie_breaking calls it
                        (:1069-1095) with reference_tiebreaking_priority (assembly_based_caller_utils.rs:197-199)
  BestAllele            new / is_informative (allele_likelihoods.rs:1142-1165)
  base quality          ReadUtils::get_read_index_for_reference_coordinate / get_read_base_quality_at_reference_coordinate
                        (src/reads/read_utils.rs:103-173), CigarUtils::cigar_consumes_* (src/reads/cigar_utils.rs:105-134)
  median                MathUtils::median (src/utils/math_utils.rs:41-45)
  normalize_sum_to_one  math_utils.rs:402-415
  annotations           VariantAnnotations::annotate / get_depth / fix_too_high_qd (src/annotator/variant_annotation.rs:93-424)
                        in the order of VariantAnnotationEngine::annotate_context (annotator/variant_annotator_engine.rs:32-113)

Plain Python floats are IEEE doubles: every comparison, subtraction and division below is the reference's."""
import numpy as np

import genotype_restatement as G

LOG_10_INFORMATIVE_THRESHOLD = 0.2     # allele_likelihoods.rs:17
EPSILON = float(np.finfo(np.float64).eps)  # f64::EPSILON
MAX_QD_BEFORE_FIXING = 45.0            # variant_annotation.rs (fix_too_high_qd :416-424)
NO_AD, NO_QD, QD_JITTER = 1, 2, 4      # PHMM_ANN_* (include/phmm.h)
NEG_INF = float("-inf")
CIGAR_OPS = "MIDNSHP=X"                # BAM codes 0..8


def encode_cigar(text):
    """'3S10M2D' -> BAM-encoded elements (length << 4 | op)."""
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append(int(n) << 4 | CIGAR_OPS.index(ch))
            n = ""
    return np.array(out, np.uint32)


def reference_tiebreaking_priority(call_allele_index):
    """1 for the reference allele (entry 0 of a call), 0 otherwise."""
    return 1 if call_allele_index == 0 else 0


def search_best_allele(values, priorities):
    """allele_likelihoods.rs:457-554 for one unit of evidence: `values` its likelihood per allele (len >= 1),
    can_be_reference = true -> (best allele, best likelihood, second best likelihood)."""
    allele_count = len(values)
    best_allele_index = 0                                       # :479-484 (can_be_reference)
    second_best_index = 0
    best_likelihood = values[best_allele_index]
    second_best_likelihood = NEG_INF
    for a in range(best_allele_index + 1, allele_count):        # :490-505
        candidate_likelihood = values[a]
        if candidate_likelihood > best_likelihood:
            second_best_index = best_allele_index
            best_allele_index = a
            second_best_likelihood = best_likelihood
            best_likelihood = candidate_likelihood
        elif candidate_likelihood > second_best_likelihood:
            second_best_index = a
            second_best_likelihood = candidate_likelihood
    if priorities is not None:                                  # :507-538
        if (best_likelihood - second_best_likelihood) < LOG_10_INFORMATIVE_THRESHOLD:
            best_priority = priorities[best_allele_index]
            second_best_priority = priorities[second_best_index]
            for a in range(allele_count):
                candidate_likelihood = values[a]
                if a == best_allele_index or (best_likelihood - candidate_likelihood) > LOG_10_INFORMATIVE_THRESHOLD:
                    continue
                candidate_priority = priorities[a]
                if candidate_priority > best_priority:
                    second_best_index = best_allele_index
                    best_allele_index = a
                    second_best_priority = best_priority
                    best_priority = candidate_priority
                elif candidate_priority > second_best_priority:
                    second_best_index = a
                    second_best_priority = candidate_priority
    best_likelihood = values[best_allele_index]                 # :540-545
    second_best_likelihood = values[second_best_index] if second_best_index != best_allele_index else NEG_INF
    return best_allele_index, best_likelihood, second_best_likelihood


def best_allele(values, priorities):
    """search_best_allele + BestAllele::new (:1142-1160) -> (allele, likelihood, confidence)."""
    values = [float(v) for v in values]
    index, likelihood, second = search_best_allele(values, priorities)
    d = likelihood - second
    confidence = 0.0 if abs(d) < EPSILON else d
    return index, likelihood, confidence


def is_informative(confidence):
    """:1163."""
    return confidence > LOG_10_INFORMATIVE_THRESHOLD


def cigar_consumes_read_bases(op):
    return CIGAR_OPS[op] in "M=XIS"          # cigar_utils.rs:105-115


def cigar_consumes_reference_bases(op):
    return CIGAR_OPS[op] in "MDN=X"          # cigar_utils.rs:117-127


def get_read_index_for_reference_coordinate(alignment_start, cigar, ref_coord):
    """read_utils.rs:103-148 -> (read index or None, op or None)."""
    if ref_coord < alignment_start:
        return None, None
    last_read_pos_of_element = 0
    last_ref_pos_of_element = alignment_start
    for el in cigar:
        length, op = int(el) >> 4, int(el) & 15
        first_read_pos_of_element = last_read_pos_of_element
        first_ref_pos_of_element = last_ref_pos_of_element
        last_read_pos_of_element += length if cigar_consumes_read_bases(op) else 0
        last_ref_pos_of_element += length if (cigar_consumes_reference_bases(op) or CIGAR_OPS[op] == "S") else 0
        if first_ref_pos_of_element <= ref_coord < last_ref_pos_of_element:
            read_pos_at_ref_coord = first_read_pos_of_element + \
                ((ref_coord - first_ref_pos_of_element) if cigar_consumes_read_bases(op) else 0)
            return read_pos_at_ref_coord, op
    return None, None


def get_read_base_quality_at_reference_coordinate(start, end, soft_start, cigar, quals, ref_coord):
    """read_utils.rs:150-173: None, or the quality at the read index the walk gives."""
    if ref_coord < start or end < ref_coord:
        return None
    offset, op = get_read_index_for_reference_coordinate(soft_start, cigar, ref_coord)
    if op is None:
        return None
    if cigar_consumes_read_bases(op):
        return int(quals[offset])
    return None


def median(numbers):
    """MathUtils::median: sort, the element at len / 2 (the upper median of an even count)."""
    numbers = sorted(numbers)
    return numbers[len(numbers) // 2]


def normalize_sum_to_one(array):
    """math_utils.rs:402-415; a zero sum divides 0.0 by 0.0 (NaN), as f64 does."""
    if len(array) == 0:
        return array
    total = 0.0
    for x in array:
        total += x
    assert total >= 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        return [float(np.float64(x) / np.float64(total)) for x in array]


def get_depth(called, ads, evidence_count):
    """variant_annotation.rs:360-405.  called[s]: the genotype is het / hom-var / hom-ref; ads[s]: its AD or None (has_ad is
    false); evidence_count[s]: likelihoods.sample_evidence_count (the used reads and the filtered ones appended to them)."""
    depth = 0
    ad_restrict_depth = 0
    for s in range(len(called)):
        if not called[s]:
            continue
        if ads[s] is not None and len(ads[s]) > 0:
            total_ad = sum(int(x) for x in ads[s])
            if total_ad != 0:
                if total_ad - int(ads[s][0]) > 0:
                    ad_restrict_depth += total_ad
                depth += total_ad
                continue
        depth += int(evidence_count[s])
    if ad_restrict_depth > 0:
        depth = ad_restrict_depth
    return depth


def has_log10_p_error(e):
    """variant_context.rs:230-232; NaN is the C ABI's way to say that there is none."""
    return not np.isnan(e) and abs(e - 1.0) > EPSILON


def annotate_event(L, keep, read_sample, read_start, read_end, mapq, n_samples, n_alleles, hap_allele, w0, w1, call,
                   log10_p_error, called=None, n_filtered=None, aligned=None):
    """One event.  L [reads, haps] of its region; call: indices of the call's alleles among the event's; aligned: None or
    (quals per read, cigar per read, soft_start per read, event position) -> dict of the outputs of phmm_annotate_events."""
    C, S = len(call), n_samples
    if C == 0:  # not annotated
        return dict(ad=np.zeros((S, 0), np.int32), af=np.zeros((S, 0)), dp=np.zeros(S, np.int32), ac=np.zeros(S, np.uint32),
                    mq=np.zeros(0, np.uint8), bq=None if aligned is None else np.zeros(0, np.uint8), info_dp=0, qd_depth=0, qd=0.0, flags=0)
    keep = np.ones(L.shape[0], bool) if keep is None else np.asarray(keep) != 0
    M_all = G.marginalize(L, hap_allele, n_alleles)
    priorities = [reference_tiebreaking_priority(c) for c in range(C)]
    used, best = [], []
    for s in range(S):  # retain_evidence, then the rows of the call's alleles; best_alleles_tie_breaking per sample
        u = np.flatnonzero(keep & (read_sample == s) & G.overlaps(w0, w1, read_start, read_end))
        values = M_all[list(call)][:, u]
        used.append(u)
        best.append([best_allele(values[:, j], priorities) for j in range(len(u))])
    flags = 0
    # ---- FORMAT: Depth (-> DepthPerAlleleBySample), AlleleFraction, AlleleCount (variant_annotator_engine.rs:103-113) ----
    ads = []
    for s in range(S):
        if C <= 1:                                                 # :250-252: returns before AD is set
            ads.append(None)
            continue
        counts = [0] * C
        for index, _, confidence in best[s]:
            if is_informative(confidence):
                counts[index] += 1
        ads.append(counts)
    if C <= 1:
        flags |= NO_AD
    ad = np.array([a if a is not None else [0] * C for a in ads], np.int32).reshape(S, C)
    dp = np.array([sum(a) if a is not None else 0 for a in ads], np.int32)                    # :115-116
    af = np.array([normalize_sum_to_one([float(x) for x in a]) if a is not None else [0.0] * C for a in ads], np.float64).reshape(S, C)
    ac = np.array([sum(1 for x in a if x > 0) if a is not None else 0 for a in ads], np.uint32)  # :162-171
    # ---- INFO: Depth, QualByDepth, MappingQuality, BaseQuality (:92-100) ----
    info_dp = int(sum(int(x) for x in dp))                         # genotype_builder.rs:502-504
    called = [True] * S if called is None else [bool(x) for x in called]
    evidence = [len(used[s]) + (0 if n_filtered is None else int(n_filtered[s])) for s in range(S)]
    depth = get_depth(called, ads, evidence)
    qd = 0.0
    if not has_log10_p_error(log10_p_error) or S == 0 or depth == 0:   # :302-315
        flags |= NO_QD
    else:
        qual = -10.0 * float(log10_p_error)
        qd = qual / float(depth)
        if not qd < MAX_QD_BEFORE_FIXING:                          # fix_too_high_qd draws from a thread RNG: the caller's
            flags |= QD_JITTER

    def statistic(value_of):                                       # :188-236
        values = {}
        for s in range(S):
            for j, (index, _, confidence) in enumerate(best[s]):
                r = int(used[s][j])
                if is_informative(confidence) and int(mapq[r]) != 0:
                    v = value_of(r)
                    values.setdefault(index, [])
                    if v is not None:
                        values[index].append(v)
        return np.array([median(values[c]) if len(values.get(c, [])) > 0 else 30 for c in range(C)], np.uint8)

    mq = statistic(lambda r: int(mapq[r]))
    bq = None
    if aligned is not None:
        quals, cigars, soft_start, pos = aligned
        bq = statistic(lambda r: get_read_base_quality_at_reference_coordinate(
            int(read_start[r]), int(read_end[r]), int(soft_start[r]), cigars[r], quals[r], int(pos)))
    return dict(ad=ad, af=af, dp=dp, ac=ac, mq=mq, bq=bq, info_dp=info_dp, qd_depth=depth, qd=qd, flags=flags)


def batch_annotate(batch, likelihoods, keep, read_sample, read_start, read_end, mapq, n_samples, ev, call_alleles, log10_p_error,
                   sample_called=None, n_filtered=None, aligned=None, only=None):
    """annotate_event over a RegionBatch-like layout and a genotype.Events; aligned: a genotype.AlignedReads or None."""
    res = {}
    nh_of = np.diff(batch.region_hap_off.astype(np.int64))[ev.region.astype(np.int64)]
    map_off = np.concatenate([[0], np.cumsum(nh_of)])
    S = n_samples
    for e in (range(ev.n_events) if only is None else only):
        g = int(ev.region[e])
        r0, r1 = int(batch.region_read_off[g]), int(batch.region_read_off[g + 1])
        nh = int(batch.region_hap_off[g + 1] - batch.region_hap_off[g])
        L = np.asarray(likelihoods[int(batch.out_off[g]):int(batch.out_off[g]) + (r1 - r0) * nh]).reshape(r1 - r0, nh)
        moff = int(map_off[e])
        al = None
        if aligned is not None:
            quals = [aligned.base_q[int(aligned.read_off[r]):int(aligned.read_off[r + 1])] for r in range(r0, r1)]
            cigars = [aligned.cigar[int(aligned.cigar_off[r]):int(aligned.cigar_off[r]) + int(aligned.n_cigar[r])] for r in range(r0, r1)]
            al = (quals, cigars, aligned.soft_start[r0:r1], int(aligned.event_pos[e]))
        res[e] = annotate_event(
            L, None if keep is None else keep[r0:r1], read_sample[r0:r1], read_start[r0:r1], read_end[r0:r1], mapq[r0:r1], S,
            ev.n_alleles(e), ev.hap_allele[moff:moff + nh], int(ev.start[e]), int(ev.end[e]), list(call_alleles[e]),
            float(log10_p_error[e]), None if sample_called is None else np.asarray(sample_called).reshape(-1, S)[e],
            None if n_filtered is None else np.asarray(n_filtered).reshape(-1, S)[e], al)
    return res
