"""The restatement of the reference's genotype assignment (tests/assign_restatement.py) against the reference's own
expectations and hand-derived cases, on the CPU: every case of make_update_pls_sacs_and_ad_data that carries PLs
(tests/golden/subset_alleles_cases.json), the subset index table, is_informative at its boundary, the first-maximum rule with
the `>=` scan of the GQ, get_gq_log10_from_posteriors in each of its five arms, the prior tables, the QUAL update -- and that
the seeds of the GPU tests keep their skipped cases within the cap, and that the binding declares the call."""
import ctypes as C
import json
import math
import os
import re

import pytest

import assign_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "subset_alleles_cases.json")))["cases"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "line%d" % c["line"])
def test_reference_subsetting_cases(case):
    """Original PLs (as_pls of the case's log10 likelihoods), kept alleles -> the expected genotype's PLs, and its GQ where
    subset_alleles ran."""
    pls = R.gls_to_pls(case["log10_likelihoods"])
    want = R.gls_to_pls(case["expected_log10_likelihoods"])
    kinds = [R.PLAIN] * case["n_alleles"]
    r = R.assign_event(case["ploidy"], [1] * case["n_alleles"], kinds, case["keep"], [pls])
    assert r["sub_pl"] == [want]
    if case["expected_gq"] is not None:
        assert r["gq"] == [case["expected_gq"]] and r["called"] == [1]
        best = want.index(0)
        assert r["gt"] == [R.as_allele_list(case["ploidy"], len(case["keep"]), best)]
    if not any(pls):
        assert r["flags"] == [R.UNINFORMATIVE] and r["gt"] == [[R.NO_CALL] * case["ploidy"]] and r["gq"] == [-1] and r["called"] == [0]


def test_every_case_with_pls_is_transcribed():
    assert len(CASES) == 10 and sorted(c["ploidy"] for c in CASES) == [1, 1, 1, 2, 2, 2, 2, 3, 3, 3]
    assert [c["expected_gq"] for c in CASES[4:]] == [500, 300, 400, 300, 200, 200]


def test_subset_index_table_by_hand():
    # diploid over A, B, C: AA AB BB AC BC CC -> {A, B}: AA AB BB
    assert R.subsetted_pl_indices(2, 3, [0, 1]) == [0, 1, 2]
    # diploid over four alleles: 00 01 11 02 12 22 03 13 23 33 -> {0, 2, 3}: 00 02 22 03 23 33
    assert R.subsetted_pl_indices(2, 4, [0, 2, 3]) == [0, 3, 5, 6, 8, 9]
    # triploid over three: 000 001 011 111 002 012 112 022 122 222 -> {0, 2}: 000 002 022 222
    assert R.subsetted_pl_indices(3, 3, [0, 2]) == [0, 4, 7, 9]
    for ploidy, A in ((1, 5), (2, 5), (3, 4), (5, 3)):
        assert R.subsetted_pl_indices(ploidy, A, list(range(A))) == list(range(len(R.G.genotypes(ploidy, A))))


def test_is_informative_at_its_boundary():
    """0 / -10 + 1 / -10 + 0 / -10 = -0.1, which is not below -0.1."""
    assert not R.is_informative(R.pls_to_gls([0, 0, 0])) and not R.is_informative(R.pls_to_gls([0, 1, 0]))
    assert R.is_informative(R.pls_to_gls([0, 1, 1])) and R.is_informative(R.pls_to_gls([0, 2, 0]))
    r = R.assign_event(2, [1, 1], [0, 0], [0, 1], [[0, 1, 0], [0, 1, 1]])
    assert r["gt"] == [[-1, -1], [0, 0]] and r["gq"] == [-1, 1] and r["called"] == [0, 1] and r["flags"] == [R.UNINFORMATIVE, 0]
    assert r["sub_pl"] == [[0, 1, 0], [0, 1, 1]]  # emit_empty_pls: the PLs are set either way


def test_first_maximum_and_the_scan_of_the_gq():
    # two equal best: the first is chosen, the other is the best of the rest through `>=`, so GQ is 0
    r = R.assign_event(2, [1, 1, 1], [0] * 3, [0, 1, 2], [[40, 0, 40, 0, 40, 40], [7] * 6, [30, 20, 20, 0, 90, 90]])
    assert r["gt"] == [[0, 1], [0, 0], [0, 2]] and r["gq"] == [0, 0, 20]
    assert R.get_gq_log10_from_likelihoods(1, [-3.0, 0.0, -2.0, -2.0]) == -2.0
    # a chosen index that is not the maximum takes the normalising arm (never from subset_alleles)
    got = R.get_gq_log10_from_likelihoods(1, [0.0, -1.0])
    assert abs(got - math.log10(1.0 - 0.1 / 1.1)) < 1e-15
    assert R.gq_of(-2.05) == 21 and R.gq_of(-2.04999) == 20 and R.gq_of(1.0) == -10 and R.gq_of(-1e300) == R.I32_MAX  # half away, `as i32`


def test_gq_from_posteriors_in_each_arm():
    lg = math.log10
    assert R.get_gq_log10_from_posteriors(0, []) == 1.0 and R.get_gq_log10_from_posteriors(0, [0.0]) == 1.0
    assert R.get_gq_log10_from_posteriors(0, [0.0, -3.0]) == -3.0 and R.get_gq_log10_from_posteriors(1, [-2.0, 0.0]) == -2.0
    # three: the two that are not the best, wrapping around; capped at 0
    assert abs(R.get_gq_log10_from_posteriors(0, [0.0, -1.0, -2.0]) - lg(0.1 + 0.01)) < 1e-15
    assert abs(R.get_gq_log10_from_posteriors(1, [-1.0, 0.0, -2.0]) - lg(0.1 + 0.01)) < 1e-15
    assert abs(R.get_gq_log10_from_posteriors(2, [-2.0, -1.0, 0.0]) - lg(0.1 + 0.01)) < 1e-15
    assert R.get_gq_log10_from_posteriors(0, [0.0, 0.0, 0.0]) == 0.0
    # general: the best first, last, and inside (the two sides summed, capped at 0)
    p = [0.0, -1.0, -2.0, -3.0]
    assert abs(R.get_gq_log10_from_posteriors(0, p) - lg(0.111)) < 1e-15
    assert abs(R.get_gq_log10_from_posteriors(3, p[::-1]) - lg(0.111)) < 1e-15
    assert abs(R.get_gq_log10_from_posteriors(1, [-1.0, 0.0, -2.0, -3.0]) - lg(0.1 + 0.011)) < 1e-15
    assert R.get_gq_log10_from_posteriors(2, [0.0, 0.0, 0.0, 0.0, 0.0]) == 0.0


def test_prior_tables_and_allele_types():
    het, hom, diff = R.assuming_hw(-3.0, -4.0)
    assert het == [0.0, -3.0 - math.log10(3.0), -4.0, -3.0] and hom == [0.0, -6.0 - math.log10(3.0), -8.0, -6.0]
    assert diff[2] == -4.0 and diff[0] == 0.0
    # '*' is typed by its length like any other allele; <NON_REF> makes the reference panic
    assert R.calculate_allele_types([2, 2, 1, 5], [R.PLAIN, R.PLAIN, R.SPAN_DEL, R.PLAIN]) == [R.REF, R.SNP, R.INDEL, R.INDEL]
    with pytest.raises(ValueError):
        R.calculate_allele_types([1, 0], [R.PLAIN, R.NON_REF])
    # diploid REF / SNP / INDEL: 00 01 11 02 12 22; triploid counts go through het + diff * (count - 1)
    pr = R.log10_priors((het, hom, diff), 2, [R.REF, R.SNP, R.INDEL])
    assert pr == [0.0, 0.0 + het[1], hom[1], 0.0 + het[2], het[1] + het[2], hom[2]]
    pr3 = R.log10_priors((het, hom, diff), 3, [R.REF, R.INDEL])
    assert pr3 == [0.0, 0.0 + het[2], 0.0 + hom[2], het[2] + diff[2] * 2.0]


def test_posterior_call_and_qual_update():
    r = R.assign_event(2, [1, 1, 2], [0, 0, 0], [0, 2], [[50, 10, 0, 40, 30, 60]], R.USE_POSTERIORS, -3.0, math.log10(1.25e-4))
    # likelihoods -5 -4 -6; the indel priors 0, log10(1.25e-4), twice that: the reference genotype wins
    assert r["gt"] == [[0, 0]] and r["called"] == [1] and r["flags"] == [0] and r["sub_pl"] == [[10, 0, 20]]
    assert r["gp"][0][0] == 0.0 and abs(r["gp"][0][1] - (-10.0 * (-4.0 + math.log10(1.25e-4) + 5.0))) < 1e-12
    assert r["pg"][0] == [0.0, -10.0 * math.log10(1.25e-4), -10.0 * (math.log10(1.25e-4) * 2.0)]
    assert r["gq"] == [29]
    # no '*': posteriors[0] - max(0, phred_sum); here posteriors[0] is 0 and the sum is just below it
    assert r["qual_update"] == 0.0
    # with a '*' in the call and ploidy 2 the "non variant" values are posteriors[0] and posteriors[1], as written
    gp = [3.0, 0.0, 40.0]
    want = max(0.0, R.phred_sum(gp[:2])) - max(0.0, R.phred_sum(gp))
    assert R.extract_p_no_alt_with_posteriors([R.PLAIN, R.SPAN_DEL], 2, gp) == want
    # ref only and not called: no update, zeros
    assert math.isnan(R.assign_event(2, [1, 1], [0, 0], [0], [[0, 5, 9]], R.USE_POSTERIORS)["qual_update"])
    assert R.assign_event(2, [1, 1], [0, 0], [0], [[0, 5, 9]])["flags"] == [R.REF_ONLY]
    assert R.assign_event(2, [1, 1], [0, 0], [], [[0, 5, 9]])["called"] == [0]


def test_determine_type():
    assert [R.determine_type(a) for a in ([], [-1, -1], [-1, 0], [0, 1], [0, 0], [2, 2], [0, 0, 1])] == \
        ["Unavailable", "NoCall", "Mixed", "Het", "HomRef", "HomVar", "Het"]


def test_gpu_test_seeds_stay_within_the_skip_cap():
    """What tests/test_assign_hip.py::test_posterior_method_grid leaves out for sitting on a decision boundary."""
    import test_assign_hip as T
    drawn = skipped = 0
    for ploidy, S, events in T.posterior_events(T.POSTERIOR_SEED):
        for ev in events:
            drawn += 1
            skipped += T.want_of(ev, ploidy, R.USE_POSTERIORS)["margin"] < T.MARGIN
    assert drawn >= 300 and skipped <= T.MAX_SKIPPED * drawn, (drawn, skipped)


def test_gpu_boundary_shapes_skip_nothing():
    """tests/test_assign_edges_hip.py::test_wave_and_block_boundaries compares every event it draws with the posterior method:
    none of them is within the margin of a decision boundary."""
    import test_assign_edges_hip as E
    import test_assign_hip as T
    for ploidy, A, C in E.BOUNDARY_SHAPES:
        margins = [T.want_of(ev, ploidy, R.USE_POSTERIORS)["margin"] for ev in E.boundary_events(ploidy, A, C)]
        assert len(margins) == 2 and min(margins) >= T.MARGIN, ((ploidy, A, C), margins)


def test_binding_declares_the_call():
    from lorikeet_amd import _lib
    sym = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    assert "phmm_assign_genotypes" in sym
    res, args = sym["phmm_assign_genotypes"]
    header = open(os.path.join(HERE, "..", "include", "phmm.h")).read()
    decl = re.search(r"int phmm_assign_genotypes\((.*?)\);", header, re.S).group(1)
    assert res is C.c_int and len(args) == len(decl.split(",")) == 25
    assert (_lib.PHMM_GT_USE_PLS, _lib.PHMM_GT_USE_POSTERIORS) == (R.USE_PLS, R.USE_POSTERIORS)
    assert (_lib.PHMM_GT_SAMPLE_UNINFORMATIVE, _lib.PHMM_GT_SAMPLE_NON_REF_BEST, _lib.PHMM_GT_SAMPLE_REF_ONLY) == \
        (R.UNINFORMATIVE, R.NON_REF_BEST, R.REF_ONLY)
