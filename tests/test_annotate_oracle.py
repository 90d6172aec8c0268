"""CPU checks of the annotation step (phmm_annotate_events, include/phmm.h): the restatement the device is held to
(tests/annotate_restatement.py) pinned piece by piece -- search_best_allele against the best-allele oracle
(oracle/engine_oracle.c, itself pinned by the reference's property test in tests/test_best_alleles_oracle.py), the CIGAR
walk against cases derived by hand from src/reads/read_utils.rs:103-173, the upper median, get_depth branch by branch."""
import numpy as np
import pytest

import annotate_restatement as A
from oracle import oracle

THR = 0.2


def _planted(rng, n_alleles, n_reads):
    """N(0, 1) likelihoods; then per read one of: as drawn, an exact tie with the best, another allele at exactly best - 0.2,
    one ulp inside it, one ulp outside it, the reference that far from the best, -inf entries, a row of -inf."""
    v = rng.normal(0.0, 1.0, size=(n_alleles, n_reads))
    for r in range(n_reads):
        kind = r % 9
        b = int(np.argmax(v[:, r]))
        other = int(rng.integers(0, n_alleles))
        gap = [None, 0.0, THR, np.nextafter(THR, 0.0), np.nextafter(THR, 1.0)][kind] if kind < 5 else None
        if gap is not None and other != b:
            v[other, r] = v[b, r] - gap
        elif kind == 5 and b != 0:
            v[0, r] = v[b, r] - [THR, np.nextafter(THR, 0.0), np.nextafter(THR, 1.0), 0.0][r // 9 % 4]
        elif kind == 6:
            v[rng.random(n_alleles) < 0.5, r] = -np.inf
        elif kind == 7:
            v[:, r] = -np.inf
        elif kind == 8:
            v[:, r] = np.round(v[:, r] * 5) / 5  # many differences of 0.2 (as rounded) and ties
    return v


@pytest.mark.parametrize("n_alleles", [1, 2, 3, 5, 8, 17, 44])
def test_search_best_allele_equals_the_oracle(n_alleles):
    rng = np.random.default_rng(n_alleles)
    v = _planted(rng, n_alleles, 900)
    pri = [A.reference_tiebreaking_priority(a) for a in range(n_alleles)]
    best, lk, conf = oracle.best_alleles(v, pri, THR)
    informative = 0
    for r in range(v.shape[1]):
        b, likelihood, confidence = A.best_allele(v[:, r], pri)
        assert b == best[r], (r, v[:, r])
        assert likelihood == lk[r] or (np.isnan(likelihood) and np.isnan(lk[r]))
        assert confidence == conf[r] or (np.isnan(confidence) and np.isnan(conf[r])), (r, v[:, r], confidence, conf[r])
        informative += A.is_informative(confidence)
    assert n_alleles == 1 or 0 < informative < v.shape[1]


def test_the_threshold_is_strict_on_both_sides():
    lo, hi = float(np.nextafter(THR, 0.0)), float(np.nextafter(THR, 1.0))
    # the second best exactly 0.2 below: not < 0.2, so no tie-breaking; the confidence 0.2 is not > 0.2: not informative
    for gap, informative in ((THR, False), (hi, True), (lo, False)):
        b, _, c = A.best_allele([-gap, 0.0], [1, 0])  # allele 1 best; the reference `gap` below (0.0 - -gap is exact)
        if gap == lo:
            assert b == 0 and c == -lo  # inside the threshold the reference takes over, with a negative confidence
        else:
            assert b == 1 and c == gap
        assert A.is_informative(c) == informative
    # one allele: the second best is -inf, the confidence +inf unless the likelihood is -inf too (NaN: not informative)
    assert A.best_allele([-3.0], [1]) == (0, -3.0, float("inf"))
    assert np.isnan(A.best_allele([-np.inf], [1])[2]) and not A.is_informative(A.best_allele([-np.inf], [1])[2])


# The walk of read_utils.rs:103-148 over 2H 3S 5M 2I 4M 3D 6M 2N 3M 4S from the soft start 100, element by element
# ([first, last) on the read | on the reference; a soft clip advances both, H and an insertion leave the reference where it is):
#   2H  read [0,0)    ref [100,100)      3S  read [0,3)    ref [100,103)      5M  read [3,8)    ref [103,108)
#   2I  read [8,10)   ref [108,108)      4M  read [10,14)  ref [108,112)      3D  read [14,14)  ref [112,115)
#   6M  read [14,20)  ref [115,121)      2N  read [20,20)  ref [121,123)      3M  read [20,23)  ref [123,126)
#   4S  read [23,27)  ref [126,130)
# The index is first_read + (coordinate - first_ref) in an element that consumes read bases, first_read otherwise (:136-142).
# get_start is 103 (behind the clip) and get_end 103 + (5 + 4 + 3 + 6 + 2 + 3) - 1 = 125; quals[i] = 10 + i.
CIGAR = A.encode_cigar("2H3S5M2I4M3D6M2N3M4S")
WALK = [(99, None, None), (100, 0, "S"), (102, 2, "S"), (103, 3, "M"), (107, 7, "M"), (108, 10, "M"), (111, 13, "M"),
        (112, 14, "D"), (114, 14, "D"), (115, 14, "M"), (120, 19, "M"), (121, 20, "N"), (122, 20, "N"), (123, 20, "M"),
        (125, 22, "M"), (126, 23, "S"), (129, 26, "S"), (130, None, None)]
QUALITY = {99: None, 100: None, 102: None,   # before get_start: in the leading soft clip or before it (:154)
           103: 13, 107: 17, 108: 20, 111: 23, 112: None, 114: None,  # inside the deletion: an element without read bases (:166-170)
           115: 24, 120: 29, 121: None, 123: 30, 125: 32,
           126: None, 130: None}             # past get_end (:154)


@pytest.mark.parametrize("coord,index,op", WALK)
def test_cigar_walk_hand_derived(coord, index, op):
    got_index, got_op = A.get_read_index_for_reference_coordinate(100, CIGAR, coord)
    assert got_index == index and (got_op is None if op is None else A.CIGAR_OPS[got_op] == op)


def test_base_quality_hand_derived():
    quals = np.arange(10, 37, dtype=np.uint8)  # 27 read bases: 3S + 5M + 2I + 4M + 6M + 3M + 4S
    for coord, want in QUALITY.items():
        assert A.get_read_base_quality_at_reference_coordinate(103, 125, 100, CIGAR, quals, coord) == want, coord
    # 10M at 50: both ends, one before, one past
    m = A.encode_cigar("10M")
    assert [A.get_read_base_quality_at_reference_coordinate(50, 59, 50, m, quals, c) for c in (49, 50, 59, 60)] == [None, 10, 19, None]
    # = and X consume both; a hard clip neither: 2H 2= 1X 2= from 7 -> coordinate 9 is read index 2
    assert A.get_read_base_quality_at_reference_coordinate(7, 11, 7, A.encode_cigar("2H2=1X2="), quals, 9) == 12
    # a deletion as the last element: inside it, None (3M 2D from 10: get_end = 14)
    assert A.get_read_base_quality_at_reference_coordinate(10, 14, 10, A.encode_cigar("3M2D"), quals, 13) is None
    assert A.get_read_base_quality_at_reference_coordinate(10, 14, 10, A.encode_cigar("3M2D"), quals, 12) == 12
    # the coordinate before the soft start although inside [start, end] (a caller's inconsistent soft start): None (:108-110)
    assert A.get_read_base_quality_at_reference_coordinate(50, 59, 55, m, quals, 52) is None


def test_upper_median():
    assert A.median([5]) == 5
    assert A.median([9, 1, 5]) == 5                  # odd: the middle
    assert A.median([1, 9]) == 9                     # even: index len / 2, the upper of the two
    assert A.median([7, 3, 9, 1]) == 7
    assert A.median([2, 2, 8, 8, 8, 1]) == 8         # sorted 1 2 2 8 8 8 -> index 3
    assert A.median([60] * 4 + [0] * 4) == 60


def test_get_depth_branches():
    # a no-call is skipped whatever it holds
    assert A.get_depth([False, True], [[5, 5], [1, 0]], [9, 9]) == 1
    # AD-restricted: only the samples with an alternate read count once there is one
    assert A.get_depth([True, True, True], [[4, 0], [3, 2], [0, 6]], [50, 50, 50]) == 5 + 6
    # no sample has an alternate read: every total counts
    assert A.get_depth([True, True], [[4, 0], [3, 0]], [50, 50]) == 7
    # AD all zero: the evidence count (used reads + filtered ones) stands in
    assert A.get_depth([True], [[0, 0]], [12]) == 12
    assert A.get_depth([True, True], [[0, 0], [2, 0]], [12 + 3, 40]) == 15 + 2
    # ... but not once an AD-restricted depth exists
    assert A.get_depth([True, True], [[0, 0], [2, 1]], [15, 40]) == 3
    # no AD at all (one allele in the call)
    assert A.get_depth([True, False], [None, None], [6, 7]) == 6
    assert A.get_depth([], [], []) == 0


def test_normalize_sum_to_one_divides_as_the_reference():
    assert A.normalize_sum_to_one([1.0, 2.0]) == [1.0 / 3.0, 2.0 / 3.0]
    assert all(np.isnan(x) for x in A.normalize_sum_to_one([0.0, 0.0])) and A.normalize_sum_to_one([]) == []


def test_one_event_by_hand():
    """Five reads, three event alleles of which the call keeps 0 and 2; window [10, 14]."""
    #            hap0(a0) hap1(a1) hap2(a2) hap3(a2)
    L = np.array([[-1.0, -0.1, -5.0, -3.0],    # best of the call: a0 (-1.0 vs -3.0): informative, although a1 is the matrix's best
                  [-2.0, -9.0, -2.1, -2.5],    # a2 within 0.2 of a0: the reference keeps it, confidence 0.1: not informative
                  [-4.0, -9.0, -1.0, -0.5],    # a2 (-0.5): informative
                  [-4.0, -9.0, -0.5, -1.0],    # a2: informative, mapq 0
                  [-0.5, -9.0, -4.0, -4.0]])   # a0, but outside the window
    start, end = np.array([10, 12, 0, 14, 15]), np.array([20, 12, 30, 14, 30])
    out = A.annotate_event(L, None, np.zeros(5, np.uint32), start, end, np.array([60, 50, 40, 0, 60]), 1, 3, [0, 1, 2, 2], 10, 14, [0, 2],
                           -12.0, aligned=([np.full(40, 30 + r, np.uint8) for r in range(5)], [A.encode_cigar("40M")] * 5, start, 12))
    assert out["ad"].tolist() == [[1, 2]] and out["dp"].tolist() == [3] and out["ac"].tolist() == [2] and out["info_dp"] == 3
    assert out["af"].tolist() == [[1.0 / 3.0, 2.0 / 3.0]]
    assert out["mq"].tolist() == [60, 40] and out["bq"].tolist() == [30, 32]  # read 3 (mapq 0) is left out; read 3 starts at 14 > 12 anyway
    assert out["qd_depth"] == 3 and out["qd"] == 120.0 / 3.0 and out["flags"] == 0
    assert A.annotate_event(L, None, np.zeros(5, np.uint32), start, end, np.full(5, 60), 1, 3, [0, 1, 2, 2], 10, 14, [0, 2], -13.5)["flags"] == A.QD_JITTER
    one = A.annotate_event(L, None, np.zeros(5, np.uint32), start, end, np.full(5, 60), 1, 3, [0, 1, 2, 2], 10, 14, [0], float("nan"))
    assert one["flags"] == A.NO_AD | A.NO_QD and one["ad"].tolist() == [[0]] and one["qd_depth"] == 4 and one["mq"].tolist() == [60]
