"""Test infrastructure, not product code: a statement-by-statement restatement of the reference's allele-frequency step,
what tests/test_af_hip.py holds phmm_allele_frequency to.

  calculate              AlleleFrequencyCalculator::calculate (src/model/allele_frequency_calculator.rs:198-379), with
                         effective_allele_counts (:411-450), log10_normalized_genotype_posteriors (:77-141, the
                         has_likelihoods arm: every genotype here carries PLs) and
                         genotype_indices_with_only_ref_and_span_del (:381-403)
  math                   MathUtils::log10_sum_log10 / normalize_log10 / log10_sum_log10_two_values / log10_one_minus_pow10
                         (src/utils/math_utils.rs:152-205, :302-312), NaturalLogUtils::log1mexp (natural_log_utils.rs:36-54),
                         Dirichlet::log10_mean_weights (src/utils/dirichlet.rs:59-68),
                         GenotypeAlleleCounts::log10_combination_count (genotype_allele_counts.rs:164-177)
  output subset, QUAL    GenotypingEngine::calculate_genotypes (src/genotype/genotyping_engine.rs:80-197) with
                         calculate_output_allele_subset (:390-449), passes_emit_threshold / passes_call_threshold (:376-382),
                         AFCalculationResult (src/model/allele_frequency_calculator_result.rs:105-148); no given alleles, the
                         event not covered by an upstream deletion

One scalar at a time with Python's float and `math`, so pow / log10 / lgamma / log1p are the platform libm's, as the
reference's powf / log10 are.  Two functions differ from the reference's and are not measured here: ln_gamma is statrs'
Lanczos approximation there and glibc's lgamma here, log1p the Rust `libm` crate's there and glibc's here.  Both agree to
within a few ulp; the device tolerance (1e-11 x max(1, |value|)) absorbs that, as it absorbs the device's own ocml pow / log10.

Besides the results, `calculate_genotypes` reports how close each integer or boolean decision came to its boundary (relative
margins): Delta count against 0.01 in every iteration, each count's fractional part against .5, each log10 value against its
threshold, QUAL against stand_min_conf."""
import functools
import math
import sys

import genotype_restatement as G

THRESHOLD_FOR_ALLELE_COUNT_CONVERGENCE = 0.01  # allele_frequency_calculator.rs:35
AF_EPSILON = 1.0e-10                           # AFCalculationResult::EPSILON
F64_EPSILON = sys.float_info.epsilon
MAX_ALLELES = 50                               # GenotypeLikelihoods::MAX_DIPLOID_ALT_ALLELES_THAT_CAN_BE_GENOTYPED
LOG10_E = math.log10(math.e)                   # math_utils.rs:21
LOG_10 = math.log(10.0)                        # math_utils.rs:19
INV_LOG_10 = 1.0 / LOG_10
LOG1MEXP_THRESHOLD = math.log(0.5)             # natural_log_utils.rs:9
PLAIN, SPAN_DEL, NON_REF = 0, 1, 2             # allele kinds (phmm_allele_frequency's allele_kind)
CALLED, LOW_QUAL, MONOMORPHIC, TOO_MANY_ALLELES, NOT_CONVERGED = 1, 2, 4, 8, 16
PLAUSIBLE, OUTPUT = 1, 2
NEG_INF = float("-inf")


def pseudo_counts(snp_het=0.001, indel_het=0.000125, het_stdev=0.01):
    """make_calculator (allele_frequency_calculator.rs:53-75): (ref, snp, indel)."""
    ref = snp_het / (het_stdev ** 2.0)
    return ref, snp_het * ref, indel_het * ref


def _sum(values):
    """Rust's Iterator::sum::<f64>: in order, from zero."""
    s = 0.0
    for v in values:
        s += v
    return s


def log10_factorial(n):
    return math.lgamma(n + 1.0) * LOG10_E


def log10_combination_count(ploidy, counts):
    return _log10_combination_count(ploidy, tuple(counts))


@functools.lru_cache(maxsize=None)
def _log10_combination_count(ploidy, counts):
    return log10_factorial(float(ploidy)) - _sum(log10_factorial(float(c)) for c in counts)


def max_element_index(values):
    m = 0
    for i in range(1, len(values)):
        if values[i] > values[m]:
            m = i
    return m


def log10_sum_log10(values):
    """math_utils.rs:161-197: the max element skipped, no log term when |sum - 1| <= f64::EPSILON."""
    if not values:
        return NEG_INF
    imax = max_element_index(values)
    mx = values[imax]
    if mx == NEG_INF:
        return mx
    sum_tot = 1.0 + _sum(10.0 ** (v - mx) for i, v in enumerate(values) if i != imax and v != NEG_INF)
    assert not (math.isnan(sum_tot) or sum_tot == math.inf)
    return mx + (math.log10(sum_tot) if abs(sum_tot - 1.0) > F64_EPSILON else 0.0)


def log10_sum_log10_two_values(a, b):
    if a > b:
        return a + math.log10(1.0 + 10.0 ** (b - a))
    return b + math.log10(1.0 + 10.0 ** (a - b))


def log1mexp(a):
    if a > 0.0:
        return math.nan
    if a == 0.0:
        return NEG_INF
    if a < LOG1MEXP_THRESHOLD:
        return math.log1p(-math.exp(a))
    return math.log(-math.expm1(a))


def log10_one_minus_pow10(a):
    if a > 0.0:
        return math.nan
    if a == 0.0:
        return NEG_INF
    return log1mexp(a * LOG_10) * INV_LOG_10


def round_half_away(x):
    return float(G.round_half_away(x))


def prior_classes(allele_length, pseudo):
    """:205-217: allele 0 the reference; same length as the reference -> SNP; otherwise indel (<FAKE_ALT>, length 0, against
    N is an indel)."""
    ref, snp, indel = pseudo
    return [ref if i == 0 else (snp if n == allele_length[0] else indel) for i, n in enumerate(allele_length)]


def normalized_posteriors(ploidy, pls, log10_af):
    """:77-141 with likelihoods pl / -10.0 (Genotype::get_likelihoods, genotype_likelihoods.rs:80-85)."""
    gts = G.genotypes(ploidy, len(log10_af))
    post = []
    for g, (alleles, counts) in enumerate(gts):
        post.append(log10_combination_count(ploidy, counts) + (pls[g] / -10.0)
                    + _sum(float(c) * log10_af[a] for a, c in zip(alleles, counts)))
    s = log10_sum_log10(post)
    return [x - s for x in post]


def effective_allele_counts(samples, log10_af):
    """:411-450; samples: [(ploidy, pls)]."""
    A = len(log10_af)
    r = [NEG_INF] * A
    for ploidy, pls in samples:
        post = normalized_posteriors(ploidy, pls, log10_af)
        for g, (alleles, counts) in enumerate(G.genotypes(ploidy, A)):
            for a, c in zip(alleles, counts):
                r[a] = log10_sum_log10_two_values(r[a], post[g] + math.log10(float(c)))
    return [10.0 ** x for x in r]


def calculate(samples, allele_length, allele_kind, pseudo, max_iterations=None):
    """AlleleFrequencyCalculator::calculate.  Returns a dict: counts (float), mle (int, reference included),
    log10_p_no_variant, log10_p_absent (reference slot 0.0), iterations, count_diffs (Delta count of every iteration)."""
    A = len(allele_length)
    assert A >= 2
    prior = prior_classes(allele_length, pseudo)
    counts = [0.0] * A
    flat = -math.log10(float(A))
    log10_af = [flat] * A
    diff = math.inf
    diffs, it = [], 0
    while diff > THRESHOLD_FOR_ALLELE_COUNT_CONVERGENCE:
        if max_iterations is not None and it == max_iterations:
            break
        new = effective_allele_counts(samples, log10_af)
        diff = max(abs(a - b) for a, b in zip(counts, new))
        diffs.append(diff)
        it += 1
        counts = new
        posterior = [p + c for p, c in zip(prior, counts)]
        total = _sum(posterior)
        log10_af = [math.log10(x / total) for x in posterior]

    span_del = [i for i, k in enumerate(allele_kind) if k == SPAN_DEL]
    p_absent = [0.0] * A
    p_no_variant = 0.0
    for ploidy, pls in samples:
        post = normalized_posteriors(ploidy, pls, log10_af)
        gts = G.genotypes(ploidy, A)
        if not span_del:
            p_no_variant += post[0]
        else:
            sd = span_del[0]
            off = G.offset_table(ploidy, A)
            idx = [G.alleles_to_index([0] * (ploidy - n) + [sd] * n, off) for n in range(ploidy + 1)]
            p_no_variant += min(0.0, log10_sum_log10([post[i] for i in idx]))
        if A == 2 and not span_del:
            continue
        absent = [[] for _ in range(A)]
        for g, (alleles, _) in enumerate(gts):
            for a in range(A):
                if a not in alleles:
                    absent[a].append(post[g])
        for a in range(A):
            p_absent[a] += min(0.0, log10_sum_log10(absent[a]))
    if A == 2 and not span_del:
        p_absent[1] = p_no_variant
    p_absent[0] = 0.0  # (the reference's own slot is never reported)
    return dict(counts=counts, mle=[int(round_half_away(c)) for c in counts], log10_p_no_variant=p_no_variant,
                log10_p_absent=p_absent, iterations=it, count_diffs=diffs)


def _rel(x, boundary):
    if math.isinf(x) or math.isnan(x):
        return math.inf
    return abs(x - boundary) / max(1.0, abs(boundary))


def calculate_genotypes(samples, allele_length, allele_kind, pseudo, stand_min_conf, max_iterations=None):
    """calculate + the output allele subset and QUAL of calculate_genotypes.  Adds: log10_p_variant_present, qual, flags
    (CALLED, LOW_QUAL, MONOMORPHIC, TOO_MANY_ALLELES, NOT_CONVERGED), allele_flags (PLAUSIBLE, OUTPUT), margin (the smallest
    relative distance of a decision quantity from its boundary)."""
    A = len(allele_length)
    if A > MAX_ALLELES or not samples:
        return dict(flags=TOO_MANY_ALLELES if A > MAX_ALLELES else 0, margin=math.inf)
    r = calculate(samples, allele_length, allele_kind, pseudo, max_iterations)
    flags = NOT_CONVERGED if r["count_diffs"][-1] > THRESHOLD_FOR_ALLELE_COUNT_CONVERGENCE else 0
    margins = [abs(d - THRESHOLD_FOR_ALLELE_COUNT_CONVERGENCE) / THRESHOLD_FOR_ALLELE_COUNT_CONVERGENCE for d in r["count_diffs"]]
    margins += [abs((c - math.floor(c)) - 0.5) / max(1.0, c) for c in r["counts"]]
    threshold = stand_min_conf * -0.1  # QualityUtils::qual_to_error_prob_log10
    allele_flags = [0] * A
    monomorphic, outputs = True, []
    for a in range(1, A):
        plausible = (r["log10_p_absent"][a] + AF_EPSILON) < threshold
        margins.append(_rel(r["log10_p_absent"][a] + AF_EPSILON, threshold))
        lone_non_ref = A - 1 == 1 and allele_kind[a] == NON_REF
        spurious = allele_kind[a] == SPAN_DEL
        out = (plausible or lone_non_ref) and not spurious
        monomorphic = monomorphic and not (plausible and not spurious)
        allele_flags[a] = (PLAUSIBLE if plausible else 0) | (OUTPUT if out else 0)
        if out:
            outputs.append(a)
    pnv = r["log10_p_no_variant"]
    pvp = log10_one_minus_pow10(pnv)
    log10_confidence = (pnv + 0.0) if not monomorphic else (pvp + 0.0)
    qual = (-10.0 * log10_confidence) + 0.0
    passes_call = qual >= stand_min_conf
    margins.append(_rel(qual, stand_min_conf))
    passes_emit = (not monomorphic) and passes_call
    first_not_non_ref = not outputs or allele_kind[outputs[0]] != NON_REF
    called = not (not passes_emit and first_not_non_ref)
    flags |= (CALLED if called else 0) | (0 if passes_call else LOW_QUAL) | (MONOMORPHIC if monomorphic else 0)
    r.update(log10_p_variant_present=pvp, qual=qual, flags=flags, allele_flags=allele_flags, margin=min(margins))
    return r


def calculate_many(cases):
    """calculate_genotypes over a list of argument tuples (a process pool's unit of work)."""
    return [calculate_genotypes(*c) for c in cases]
