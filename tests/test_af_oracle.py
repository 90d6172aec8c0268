"""The restatement of the reference's allele-frequency step (tests/af_restatement.py) held, on the CPU, to every assertion of
the reference's own tests (tests/allele_frequency_calculator_unit_tests.rs, restated as cases of our own), plus the pieces
the device relies on: pseudo counts, prior classes, log10_sum_log10's epsilon branch and the combination counts."""
import math

import pytest

import af_restatement as R
import genotype_restatement as G

FAIRLY_CONFIDENT_PL, EXTREMELY_CONFIDENT_PL = 20, 1000
SNP = [1, 1, 1]  # three plain single-base alleles (A, C, G)


def obvious(ploidy, n_alleles, counts, pl):
    """PLs_for_obvious_call: `counts` as (allele, count) pairs flattened; that genotype 0, every other `pl`."""
    alleles = [a for a, c in zip(counts[::2], counts[1::2]) for _ in range(c)]
    n = G.genotype_count(ploidy, n_alleles)
    out = [pl] * n
    out[G.alleles_to_index(alleles, G.offset_table(ploidy, n_alleles))] = 0
    return ploidy, out


def calc(samples, pseudo, n_alleles=3, kinds=None):
    return R.calculate(samples, SNP[:n_alleles], kinds or [R.PLAIN] * n_alleles, pseudo)


def close(a, b, eps):
    """approx's relative_eq!(a, b, epsilon = eps) with the default max_relative (f64::EPSILON): |a - b| <= eps or relative."""
    return abs(a - b) <= eps or abs(a - b) <= R.F64_EPSILON * max(abs(a), abs(b))


def _genotypes():
    f = FAIRLY_CONFIDENT_PL
    return dict(AA=obvious(2, 3, [0, 2], f), BB=obvious(2, 3, [1, 2], f), CC=obvious(2, 3, [2, 2], f),
                AB=obvious(2, 3, [0, 1, 1, 1], f), AC=obvious(2, 3, [0, 1, 2, 1], f), BBB=obvious(3, 3, [1, 3], f),
                CCC=obvious(3, 3, [2, 3], f))


SYMMETRY_PAIRS = [("AA BB", "AA CC"), ("AA AB", "AA AC"), ("AB AB", "AC AC"), ("AA AA BB", "AA AA CC"), ("AA AB AB", "AA AC AC"),
                  ("AA BBB", "AA CCC")]
MLE_CASES = [("AA BB", [2, 0]), ("AA AB", [1, 0]), ("AB AB", [2, 0]), ("AA AA BB", [2, 0]), ("AA AB AB", [2, 0]),
             ("AA BBB", [3, 0]), ("AA BBB CCC", [3, 3]), ("AA AB AC", [1, 1]), ("AA AB AC BBB CCC", [4, 4])]


@pytest.mark.parametrize("one,two", SYMMETRY_PAIRS)
def test_symmetries(one, two):
    g = _genotypes()
    r1 = calc([g[n] for n in one.split()], (1.0, 0.1, 0.1))
    r2 = calc([g[n] for n in two.split()], (1.0, 0.1, 0.1))
    assert close(r1["log10_p_no_variant"], r2["log10_p_no_variant"], 1e-3)
    assert close(r1["log10_p_absent"][1], r2["log10_p_absent"][2], 1e-3)


@pytest.mark.parametrize("names,want", MLE_CASES)
def test_mle_counts_including_mixed_ploidy(names, want):
    g = _genotypes()
    assert calc([g[n] for n in names.split()], (1.0, 1.0, 1.0))["mle"][1:] == want


def test_many_samples_with_low_confidence():
    ab = obvious(2, 2, [0, 1, 1, 1], FAIRLY_CONFIDENT_PL)
    counts = [calc([ab] * n, (1000.0, 1.0, 1.0), n_alleles=2)["mle"][1] for n in range(1, 11)]
    assert counts[0] == 0 and counts[1] == 0 and counts[4] == 2 and counts[8] >= 3


@pytest.mark.parametrize("n", [100, 1000])
def test_many_very_confident_samples(n):
    ac = obvious(2, 3, [0, 1, 2, 1], EXTREMELY_CONFIDENT_PL)
    r = calc([ac] * n, (1.0, 1.0, 1.0))
    assert r["mle"][1] == 0 and r["mle"][2] == n
    assert close(r["log10_p_no_variant"], r["log10_p_absent"][2], n * 0.01)
    want = n * (math.log10(0.5) - EXTREMELY_CONFIDENT_PL / 10.0)
    assert close(r["log10_p_absent"][2], want, n * 0.01)


def test_approximate_multiplicative_confidence():
    # the reference's genotypes carry the triallelic PL vectors; a biallelic site reads their first three
    aa = (2, obvious(2, 3, [0, 2], FAIRLY_CONFIDENT_PL)[1][:3])
    bb = (2, obvious(2, 3, [1, 2], FAIRLY_CONFIDENT_PL)[1][:3])
    p = [calc([aa, bb] * (i + 1), (1.0, 1.0, 1.0), n_alleles=2)["log10_p_no_variant"] for i in range(10)]
    for i in range(9):
        assert close(p[i + 1] - p[i], p[0], 0.01)


@pytest.mark.parametrize("n_ref", [1, 10, 100, 1000, 10000])
def test_many_ref_samples_dont_kill_good_variant(n_ref):
    aa = obvious(2, 2, [0, 2], EXTREMELY_CONFIDENT_PL)
    ab = obvious(2, 2, [0, 1, 1, 1], EXTREMELY_CONFIDENT_PL)
    r = calc([aa] * n_ref + [ab], (1.0, 0.1, 0.1), n_alleles=2)
    assert r["log10_p_no_variant"] < -EXTREMELY_CONFIDENT_PL / 10.0 + math.log10(n_ref) + 1.0


SD3 = [R.PLAIN, R.PLAIN, R.SPAN_DEL]


def _pvp(samples, kinds, lengths=(1, 1, 1)):
    r = R.calculate(samples, list(lengths)[:len(kinds)], kinds, (1.0, 0.1, 0.1))
    return R.log10_one_minus_pow10(r["log10_p_no_variant"])


def test_spanning_deletion_is_not_considered_variant():
    span_del, low_qual_snp = (2, [50, 100, 100, 0, 100, 100]), (2, [10, 0, 40, 100, 70, 300])
    assert _pvp([span_del], SD3) < -10.0
    low = _pvp([low_qual_snp], SD3)
    both = _pvp([low_qual_snp, span_del], SD3)
    assert close(low, both, 0.1) and both < low
    haploid = _pvp([low_qual_snp, (1, [0, 100, 100])], SD3)
    assert close(haploid, both, 1e-5)
    no_span_del = _pvp([(2, [10, 0, 40]), (1, [0, 100])], [R.PLAIN, R.PLAIN])
    assert close(no_span_del, both, 1e-6)


def test_presence_of_unlikely_spanning_deletion_doesnt_affect_results():
    without = _pvp([(2, [50, 0, 50])], [R.PLAIN, R.PLAIN])
    with_sd = _pvp([(2, [50, 0, 50, 100, 100, 100])], SD3)
    assert close(with_sd, without, 1e-4)


def test_spanning_deletion_with_very_unlikely_alt_allele():
    r = R.calculate([(4, [0] + [10000] * 14)], [1, 1, 1], [R.PLAIN, R.SPAN_DEL, R.PLAIN], (1.0, 0.1, 0.1))
    assert r["log10_p_no_variant"] <= 0.0  # the min(0, .) cap: no positive log10 probability


def test_pseudo_counts_restate_make_calculator():
    from lorikeet_amd import genotype
    ref, snp, indel = genotype.pseudo_counts()
    assert (ref, snp, indel) == R.pseudo_counts()
    assert ref == 0.001 / (0.01 ** 2.0) and snp == 0.001 * ref and indel == 0.000125 * ref
    assert genotype.pseudo_counts(0.01, 0.001, 0.1) == R.pseudo_counts(0.01, 0.001, 0.1)


def test_prior_classes():
    pc = (10.0, 0.01, 0.00125)
    assert R.prior_classes([1, 1, 2, 0], pc) == [10.0, 0.01, 0.00125, 0.00125]
    assert R.prior_classes([3, 1, 3], pc) == [10.0, 0.00125, 0.01]
    assert R.prior_classes([1, 0], pc) == [10.0, 0.00125]  # N / <FAKE_ALT>: an indel


def test_log10_sum_log10_epsilon_branch_and_skipped_maximum():
    assert R.log10_sum_log10([-3.0]) == -3.0
    assert R.log10_sum_log10([0.0, -400.0]) == 0.0       # 1 + 1e-400 == 1: no log term at all
    assert R.log10_sum_log10([0.0, -15.7]) == 0.0        # 1 + 2e-16: |sum - 1| <= EPSILON
    assert R.log10_sum_log10([0.0, -15.0]) > 0.0
    assert R.log10_sum_log10([-1.0, -1.0]) == -1.0 + math.log10(2.0)  # a tie: one maximum skipped, the other counted
    assert R.log10_sum_log10([float("-inf")] * 2) == float("-inf")


@pytest.mark.parametrize("ploidy,n_alleles", [(1, 2), (2, 3), (3, 4), (4, 2), (6, 3), (10, 2)])
def test_combination_counts_over_the_genotype_table(ploidy, n_alleles):
    from lorikeet_amd import genotype
    table = genotype.genotype_allele_counts(ploidy, n_alleles)
    assert [tuple(zip(*g)) for g in table] == [(tuple(a), tuple(c)) for a, c in G.genotypes(ploidy, n_alleles)]
    for comps in table:
        want = math.factorial(ploidy)
        for _, c in comps:
            want //= math.factorial(c)
        got = R.log10_combination_count(ploidy, [c for _, c in comps])
        assert abs(got - math.log10(want)) <= 1e-13 * max(1.0, math.log10(want))


def test_flags_and_qual_of_a_clear_call():
    r = R.calculate_genotypes([(2, [200, 0, 200])] * 4, [1, 1], [R.PLAIN, R.PLAIN], R.pseudo_counts(), 30.0)
    assert r["flags"] == R.CALLED and r["allele_flags"] == [0, R.PLAUSIBLE | R.OUTPUT]
    assert r["qual"] == -10.0 * r["log10_p_no_variant"] + 0.0 and r["mle"] == [4, 4]
    ref = R.calculate_genotypes([(2, [0, 200, 200])] * 4, [1, 1], [R.PLAIN, R.PLAIN], R.pseudo_counts(), 30.0)
    assert ref["flags"] == R.MONOMORPHIC and ref["allele_flags"] == [0, 0]
    lone = R.calculate_genotypes([(2, [0, 200, 200])], [1, 0], [R.PLAIN, R.NON_REF], R.pseudo_counts(), 30.0)
    assert lone["flags"] & R.CALLED and lone["allele_flags"] == [0, R.OUTPUT]
    assert R.calculate_genotypes([(2, [0] * 1326)], [1] * 51, [0] * 51, R.pseudo_counts(), 30.0)["flags"] == R.TOO_MANY_ALLELES
