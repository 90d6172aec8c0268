"""Test infrastructure, not product code: a statement-by-statement restatement of the reference's genotype assignment, what
tests/test_assign_hip.py holds phmm_assign_genotypes to.

  subsetted_pl_indices            AlleleSubsettingUtils::subsetted_pl_indices (src/model/allele_subsetting_utils.rs:310-353)
  subset_alleles                  AlleleSubsettingUtils::subset_alleles (:161-296) as GenotypingEngine::calculate_genotypes calls it
                                  (src/genotype/genotyping_engine.rs:199-214): genotypes from build_from_likelihoods
                                  (genotype_builder.rs:135-152: PLs, no alleles, no AD, gq -1), depth = vc.get_dp(),
                                  emit_empty_pls = true; the AD arm (:274-291) is dead
  subset_to_ref_only              VariantContext::subset_to_ref_only (src/model/variant_context.rs:586-619)
  make_genotype_call              variant_context.rs:309-449, the UsePLsToAssign and UsePosteriorProbabilities arms
  is_informative                  :573-575 with SUM_GL_THRESH_NOCALL (:109)
  get_gq_log10_from_posteriors    :524-571
  pls_to_gls, gls_to_pls, get_gq_log10_from_likelihoods   src/genotype/genotype_likelihoods.rs:55-109
  gq_of                           Genotype::log10_p_error (src/genotype/genotype_builder.rs:220-222)
  determine_type                  genotype_builder.rs:399-441; sample_called: src/annotator/variant_annotation.rs:369
  assuming_hw, log10_priors, calculate_allele_types   src/genotype/genotype_prior_calculator.rs:46-80, :116-139, :169-229
  phred_sum                       src/utils/quality_utils.rs:54-72 with log10_sum_log10_three_values (math_utils.rs:214-222)
  qual_update                     genotyping_engine.rs:216-235 with phred_no_variant_posterior_probability (:252-269) and
                                  extract_p_no_alt_with_posteriors (:282-326)

One scalar at a time with Python's float and `math`, as tests/af_restatement.py, whose log-sum helpers and tolerance
(1e-11 x max(1, |value|): ocml pow / log10 against libm) this file shares.  The index order is genotype_restatement's.
`assign_event` also reports how close each decision of the posterior method came to its boundary: the gap between the two
largest posteriors and the distance of -10 x log10 GQ from a half before rounding, both relative."""
import math

import af_restatement as AF
import genotype_restatement as G

SUM_GL_THRESH_NOCALL = -0.1
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
PLAIN, SPAN_DEL, NON_REF = 0, 1, 2
USE_PLS, USE_POSTERIORS = 0, 1
UNINFORMATIVE, NON_REF_BEST, REF_ONLY = 1, 2, 4
REF, SNP, INDEL, OTHER = 0, 1, 2, 3  # AlleleType ordinals
NO_CALL = -1
NEG_INF = float("-inf")
LOG10_SNP_NORMALIZATION_CONSTANT = math.log10(3.0)


def as_i32(x):
    """Rust's `as i32` on an f64: saturating, NaN -> 0."""
    if math.isnan(x):
        return 0
    return int(min(max(x, float(I32_MIN)), float(I32_MAX)))


def subsetted_pl_indices(ploidy, n_original, keep):
    """keep: the original indices of the new alleles, in the new order."""
    off_new = G.offset_table(ploidy, len(keep))
    result = [0] * int(off_new[ploidy, len(keep)])
    for old_index, (alleles, counts) in enumerate(G.genotypes(ploidy, n_original)):
        if not all(a in keep for a in alleles):
            continue
        count_for = dict(zip(alleles, counts))
        new_alleles = []
        for new_allele, old_allele in enumerate(keep):
            new_alleles += [new_allele] * count_for.get(old_allele, 0)
        result[G.alleles_to_index(new_alleles, off_new)] = old_index
    return result


def pls_to_gls(pls):
    return [float(p) / -10.0 for p in pls]


def gls_to_pls(gls):
    adjust = NEG_INF
    for x in gls:
        adjust = max(adjust, x)
    return [min(as_i32(AF.round_half_away(-10.0 * (x - adjust))), I32_MAX) for x in gls]


def is_informative(gls):
    return AF._sum(gls) < SUM_GL_THRESH_NOCALL


def get_gq_log10_from_likelihoods(chosen, likelihoods):
    qual = NEG_INF
    for i, x in enumerate(likelihoods):
        if i == chosen:
            continue
        if x >= qual:
            qual = x
    qual = likelihoods[chosen] - qual
    if qual < 0.0:  # normalize_from_log10(.., false, false): never with the first maximum chosen
        mx = max(likelihoods)
        normalized = [10.0 ** (x - mx) for x in likelihoods]
        total = AF._sum(normalized)
        return math.log10(1.0 - normalized[chosen] / total)
    return -1.0 * qual


def gq_of(log10_p_error):
    return as_i32(AF.round_half_away(log10_p_error * -10.0))


def get_gq_log10_from_posteriors(best, post):
    n = len(post)
    if n <= 1:
        return 1.0
    if n == 2:
        return post[1] if best == 0 else post[0]
    if n == 3:
        return min(0.0, AF.log10_sum_log10_two_values(post[2 if best == 0 else best - 1], post[0 if best == 2 else best + 1]))
    if best == 0:
        return AF.log10_sum_log10(post[1:])
    if best == n - 1:
        return AF.log10_sum_log10(post[:best])
    return min(0.0, AF.log10_sum_log10_two_values(AF.log10_sum_log10(post[:best]), AF.log10_sum_log10(post[best + 1:])))


def determine_type(alleles):
    """alleles: indices into the call's alleles, NO_CALL for '.'; -> 'Unavailable', 'NoCall', 'Mixed', 'Het', 'HomRef', 'HomVar'."""
    if not alleles:
        return "Unavailable"
    saw_no_call = saw_multiple = False
    first = None
    for a in alleles:
        if a == NO_CALL:
            saw_no_call = True
        elif first is None:
            first = a
        elif a != first:
            saw_multiple = True
    if saw_no_call:
        return "NoCall" if first is None else "Mixed"
    if saw_multiple:
        return "Het"
    return "HomRef" if first == 0 else "HomVar"


def is_called_type(t):
    return t in ("Het", "HomVar", "HomRef")


def assuming_hw(snp_het, indel_het):
    """(het, hom, diff) by AlleleType ordinal, other_het = None."""
    other = max(snp_het, indel_het)
    het = [0.0, snp_het - LOG10_SNP_NORMALIZATION_CONSTANT, indel_het, other]
    hom = [0.0, snp_het * 2.0 - LOG10_SNP_NORMALIZATION_CONSTANT, indel_het * 2.0, other * 2.0]
    return het, hom, [a - b for a, b in zip(hom, het)]


def calculate_allele_types(lengths, kinds):
    """'*' is a called, non-symbolic allele of length 1; <NON_REF> is called and symbolic: the reference panics."""
    out = []
    for i, (n, k) in enumerate(zip(lengths, kinds)):
        if i == 0:
            out.append(REF)
        elif k == NON_REF:
            raise ValueError("Cannot handle symbolic structural variants at the moment")
        else:
            out.append(SNP if n == lengths[0] else INDEL)
    return out


def log10_priors(gpc, ploidy, types):
    het, hom, diff = gpc
    gts = G.genotypes(ploidy, len(types))
    result = [0.0] * len(gts)
    for g in range(1, len(gts)):
        alleles, counts = gts[g]
        result[g] = AF._sum(hom[types[a]] if c == 2 else het[types[a]] + diff[types[a]] * float(c - 1) for a, c in zip(alleles, counts))
    return result


def as_allele_list(ploidy, n_alleles, index):
    alleles, counts = G.genotypes(ploidy, n_alleles)[index]
    return [a for a, c in zip(alleles, counts) for _ in range(c)]


def make_genotype_call(ploidy, g, method, likelihoods, kinds, gpc=None, types=None):
    """g: the genotype under construction (dict with pl, gq, alleles); kinds / types: of the call's alleles."""
    n = len(kinds)
    if method == USE_PLS:
        if not is_informative(likelihoods):
            g["alleles"] = [NO_CALL] * ploidy
            g["gq"], g["log10_gq"] = -1, math.nan
            g["flags"] |= UNINFORMATIVE
            return
        best = AF.max_element_index(likelihoods)
        final = as_allele_list(ploidy, n, best)
        if any(kinds[a] == NON_REF for a in final):
            g["alleles"] = [NO_CALL] * ploidy
            g["pl"] = gls_to_pls([0.0] * len(likelihoods))
            g["flags"] |= NON_REF_BEST
        else:
            g["alleles"] = final
        if n - 1 > 0:
            g["log10_gq"] = get_gq_log10_from_likelihoods(best, likelihoods)
            g["gq"] = gq_of(g["log10_gq"])
        return
    assert method == USE_POSTERIORS
    priors = log10_priors(gpc, ploidy, types)
    posteriors = [a + b for a, b in zip(priors, likelihoods)]
    mx = max(posteriors)
    normalized = [x - mx for x in posteriors]
    g["gp"] = [0.0 if v == 0.0 else v * -10.0 for v in normalized]
    g["pg"] = [0.0 if v == 0.0 else v * -10.0 for v in priors]
    best = AF.max_element_index(posteriors)
    g["log10_gq"] = get_gq_log10_from_posteriors(best, normalized)
    g["gq"] = gq_of(g["log10_gq"])
    g["alleles"] = as_allele_list(ploidy, n, best)
    rest = sorted(posteriors, reverse=True)
    g["margin"] = min(AF._rel(rest[0] - rest[1], 0.0) if len(rest) > 1 else math.inf,
                      abs(abs(g["log10_gq"] * -10.0) % 1.0 - 0.5) / max(1.0, abs(g["log10_gq"] * -10.0)))


def subset_alleles(ploidy, n_original, keep, kinds, sample_pls, method, gpc=None, types=None):
    """-> one dict per sample: pl, alleles, gq, log10_gq, flags (and gp, pg, margin with the posterior method)."""
    indices = subsetted_pl_indices(ploidy, n_original, keep)
    expected = len(G.genotypes(ploidy, n_original))
    out = []
    for pls in sample_pls:
        g = dict(pl=list(pls), alleles=[], gq=-1, log10_gq=math.nan, flags=0, margin=math.inf)
        original = pls_to_gls(pls)
        assert len(original) == expected
        new = [original[i] for i in indices]  # (the scaled copy of :214 is discarded)
        best = AF.max_element_index(new)
        new_log10_gq = get_gq_log10_from_likelihoods(best, new)
        if new_log10_gq != NEG_INF:
            g["log10_gq"], g["gq"] = new_log10_gq, gq_of(new_log10_gq)
        g["pl"] = gls_to_pls(new)  # use_new_likelihoods: emit_empty_pls
        make_genotype_call(ploidy, g, method, new, kinds, gpc, types)
        out.append(g)
    return out


def subset_to_ref_only(ploidy, n_samples):
    return [dict(pl=[], alleles=[0] * ploidy, gq=-1, log10_gq=math.nan, flags=REF_ONLY, margin=math.inf) for _ in range(n_samples)]


def log10_sum_log10_three_values(a, b, c):
    if a >= b and a >= c:
        return a + math.log10(1.0 + 10.0 ** (b - a) + 10.0 ** (c - a))
    if b >= c:
        return b + math.log10(1.0 + 10.0 ** (a - b) + 10.0 ** (c - b))
    return c + math.log10(1.0 + 10.0 ** (a - c) + 10.0 ** (b - c))


def phred_sum(phreds):
    n = len(phreds)
    if n == 0:
        return 1.7976931348623157e308
    if n == 1:
        return phreds[0]
    if n == 2:
        return -10.0 * AF.log10_sum_log10_two_values(phreds[0] * -0.1, phreds[1] * -0.1)
    if n == 3:
        return -10.0 * log10_sum_log10_three_values(phreds[0] * -0.1, phreds[1] * -0.1, phreds[2] * -0.1)
    return -10.0 * AF.log10_sum_log10([p * -0.1 for p in phreds])


def _max0(x):
    """max(OrderedFloat(0.0), OrderedFloat(x)): NaN is the greatest."""
    return x if math.isnan(x) or x >= 0.0 else 0.0


def extract_p_no_alt_with_posteriors(kinds, ploidy, posteriors):
    if SPAN_DEL not in kinds:
        return posteriors[0] - _max0(phred_sum(posteriors))
    non_variant = [posteriors[n] for n in range(ploidy)]  # as written: the index computed beside it is not used
    return _max0(phred_sum(non_variant)) - _max0(phred_sum(posteriors))


def qual_update(kinds, ploidy, genotypes, site_is_monomorphic):
    """NaN: the reference leaves log10_p_error as it was."""
    if not any("gp" in g for g in genotypes):
        return math.nan
    acc = math.nan
    for g in genotypes:
        b = extract_p_no_alt_with_posteriors(kinds, ploidy, g["gp"]) if "gp" in g else math.nan
        if math.isnan(b):
            continue
        acc = b if math.isnan(acc) else acc + b
    log10_no_variant_posterior = acc * -0.1
    if not site_is_monomorphic:
        return log10_no_variant_posterior + 0.0
    return AF.log10_one_minus_pow10(log10_no_variant_posterior) + 0.0


def assign_event(ploidy, lengths, kinds, keep, sample_pls, method=USE_PLS, log10_snp_het=-3.0, log10_indel_het=math.log10(1.25e-4),
                 site_is_monomorphic=False):
    """One event: lengths / kinds of its alleles, keep = the call's alleles (empty: not called), sample_pls [n_samples][G].
    -> dict(sub_pl, gt, gq, log10_gq, called, flags [per sample], gp, pg, qual_update, margin)."""
    S = len(sample_pls)
    if not keep:
        return dict(sub_pl=[[] for _ in range(S)], gt=[[0] * ploidy for _ in range(S)], gq=[0] * S, log10_gq=[0.0] * S,
                    called=[0] * S, flags=[0] * S, gp=None, pg=None, qual_update=0.0, margin=math.inf)
    assert keep[0] == 0 and all(b > a for a, b in zip(keep, keep[1:]))
    k_kinds = [kinds[a] for a in keep]
    if len(keep) == 1:
        gts = subset_to_ref_only(ploidy, S)
    else:
        gpc = types = None
        if method == USE_POSTERIORS:
            gpc = assuming_hw(log10_snp_het, log10_indel_het)
            types = calculate_allele_types([lengths[a] for a in keep], k_kinds)
        gts = subset_alleles(ploidy, len(lengths), list(keep), k_kinds, sample_pls, method, gpc, types)
    update = qual_update(k_kinds, ploidy, gts, site_is_monomorphic) if method == USE_POSTERIORS else math.nan
    post = method == USE_POSTERIORS and len(keep) > 1
    return dict(sub_pl=[g["pl"] for g in gts], gt=[g["alleles"] for g in gts], gq=[g["gq"] for g in gts],
                log10_gq=[g["log10_gq"] for g in gts], called=[int(is_called_type(determine_type(g["alleles"]))) for g in gts],
                flags=[g["flags"] for g in gts], gp=[g["gp"] for g in gts] if post else None,
                pg=[g["pg"] for g in gts] if post else None, qual_update=update, margin=min([g["margin"] for g in gts] + [math.inf]))
