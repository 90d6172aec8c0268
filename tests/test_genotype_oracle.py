"""CPU checks of the genotyping step (phmm_genotype_likelihoods, include/phmm.h): the restatement the device is held to
(tests/genotype_restatement.py) against the reference's own test formula, the genotype index order, the genotype count
the library exports, and the library's host copy of the Jacobian table."""
import ctypes as C
import math

import numpy as np
import pytest

import genotype_restatement as R
from lorikeet_amd import _lib, genotype
from oracle import oracle

PLOIDY = [1, 2, 3, 20]                 # tests/genotype_likelihood_calculator_unit_tests.rs:20-28
MAXIMUM_ALLELE = [1, 2, 5, 6]
READ_COUNTS = [[10, 100, 50], [0, 100, 10, 1, 50], [1, 2, 3, 4, 20], [10, 0]]
GRID = [(p, a) for p in PLOIDY for a in MAXIMUM_ALLELE if R.genotype_count(p, a) <= 1024]  # what the reference enumerates


def _reference_formula(M, ploidy):
    """test_likelihood_calculation (:73-141): per read approximate_log10_sum_log10_vec of lk + log10(count) over the
    genotype's alleles, minus log10(ploidy), summed over the reads."""
    out = []
    for al, cn in R.genotypes(ploidy, M.shape[0]):
        per_read = []
        for r in range(M.shape[1]):
            comps = np.array([[M[a, r] + math.log10(c)] for a, c in zip(al, cn)])
            per_read.append(R.approximate_log10_sum_log10_vec(comps)[0] - math.log10(ploidy))
        out.append(sum(per_read))
    return np.array(out)


@pytest.mark.parametrize("ploidy,n_alleles", GRID)
def test_restatement_agrees_with_the_reference_test_formula(ploidy, n_alleles):
    rng = np.random.default_rng(ploidy * 100 + n_alleles)
    for counts in READ_COUNTS:
        for n in counts:
            M = -np.abs(rng.normal(0.0, 3.0, size=(n_alleles, n)))
            want = _reference_formula(M, ploidy)
            got = R.genotype_likelihoods_of(M, ploidy)
            assert got.shape == want.shape
            assert np.allclose(got, want, rtol=0, atol=1e-4), (ploidy, n_alleles, n, np.max(np.abs(got - want)))


@pytest.mark.parametrize("ploidy,n_alleles", GRID)
def test_genotype_index_order_round_trips(ploidy, n_alleles):
    """test_ploidy_and_maximum_allele (:30-71): alleles_to_index / allele_counts_to_index of every genotype is its index;
    the library's order (genotype.genotype_allele_counts) is the restatement's."""
    off = R.offset_table(ploidy, n_alleles)
    gts = R.genotypes(ploidy, n_alleles)
    assert len(gts) == R.genotype_count(ploidy, n_alleles) == genotype.genotype_count(ploidy, n_alleles)
    lib_order = genotype.genotype_allele_counts(ploidy, n_alleles)
    for i, (al, cn) in enumerate(gts):
        assert sum(cn) == ploidy and al == sorted(al)
        alleles = [a for a, c in zip(al, cn) for _ in range(c)]
        assert R.alleles_to_index(alleles, off) == i
        assert lib_order[i] == tuple(zip(al, cn))
    if ploidy == 2 and n_alleles >= 3:
        assert [tuple(a for a, c in g for _ in range(c)) for g in lib_order[:6]] == [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2)]


def test_genotype_count_is_the_recurrence_and_saturates():
    lib = _lib.load()
    for p in range(0, 65):
        for a in range(0, 65):
            want = R.genotype_count(p, a) if a else 0
            assert lib.phmm_genotype_count(p, a) == min(want, 2 ** 32 - 1), (p, a)
    assert lib.phmm_genotype_count(3, 17) == 969
    assert lib.phmm_genotype_count(1000, 1000) == 2 ** 32 - 1
    assert lib.phmm_genotype_count(2 ** 32 - 1, 2) == 2 ** 32 - 1
    assert lib.phmm_genotype_count(2 ** 32 - 1, 1) == 1
    assert lib.phmm_genotype_count(1, 2 ** 32 - 1) == 2 ** 32 - 1


def test_jacobian_table_matches_oracle_bit_for_bit():
    lib = _lib.load()
    p = _lib.f64p()
    n = lib.phmm_table_jacobian(C.byref(p))
    assert n == 80001
    got = np.ctypeslib.as_array(p, shape=(n,)).copy()
    assert np.array_equal(got.view(np.uint64), R.jacobian_table().view(np.uint64))
    f = oracle.lib().oracle_approximate_log10_sum_log10
    assert f(-1.25, -1.0) == -1.0 + got[2500]


def test_pl_conversion_edges():
    assert np.array_equal(R.gls_to_pls(np.array([-np.inf, -np.inf, -np.inf])), [0, 0, 0])
    assert np.array_equal(R.gls_to_pls(np.array([-1.0, -np.inf, -1.05])), [0, 2 ** 31 - 1, 1])  # -10 * -0.05 = 0.5 -> 1
    assert np.array_equal(R.gls_to_pls(np.array([0.0, -1e12])), [0, 2 ** 31 - 1])
    assert np.array_equal(R.round_half_away(np.array([0.5, 1.5, 2.5, -0.5, 0.49999999999999994])), [1.0, 2.0, 3.0, -1.0, 0.0])


def test_read_end_is_get_end():
    from oracle.oracle import parse_cigar
    assert genotype.read_end(100, parse_cigar("10M")) == 109
    assert genotype.read_end(100, parse_cigar("3S10M2I4D5M")) == 118
    assert genotype.read_end(100, parse_cigar("5S4I")) == 100  # no reference bases: end == start
