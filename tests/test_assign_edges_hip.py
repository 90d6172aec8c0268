"""phmm_assign_genotypes at the edges of its layout, against the restatement (tests/assign_restatement.py) with the rules of
tests/test_assign_hip.py: G' on both sides of a wave (64 lanes) and up to the cap of 1 024 genotypes, ties that only the lowest
index may win, rows at the is_informative threshold, saturated PLs, a renormalisation that shows, and <NON_REF> in the best
genotype."""
import numpy as np
import pytest

import assign_restatement as R
import genotype_restatement as G
from test_assign_hip import MAX_SKIPPED, Event, check_exact, compare_posterior, plain, run, want_of

pytestmark = pytest.mark.gpu
I32_MAX = 2 ** 31 - 1


def _keep(rng, A, C):
    return [0] + sorted(int(a) for a in rng.choice(np.arange(1, A), size=C - 1, replace=False))


BOUNDARY_SHAPES = [(1, 70, 63), (1, 70, 64), (1, 70, 65), (2, 12, 10), (2, 12, 11), (2, 44, 2), (2, 44, 43), (2, 44, 44), (1023, 2, 2)]


def distinct_pls(rng, S, n):
    """PL rows with a zero and no two values equal, so that two genotypes of one prior never tie: their posteriors differ by
    at least 0.1, and posteriors of different priors differ by an irrational amount.  Close together (steps of 1 to 7), so
    that many terms of the log sums count."""
    rows = []
    for _ in range(S):
        values = np.concatenate([[0], np.cumsum(rng.integers(1, 8, size=n - 1))])
        rows.append(rng.permutation(values))
    return rows


def boundary_events(ploidy, A, C):
    """The two events of one shape (tests/test_assign_oracle.py checks on the CPU that none of them sits on a decision
    boundary of the posterior method)."""
    rng = np.random.default_rng(A * 100 + C)
    n = G.genotype_count(ploidy, A)
    return [Event(*plain(A), _keep(rng, A, C), distinct_pls(rng, 3, n)) for _ in range(2)]


@pytest.mark.parametrize("ploidy,A,C", BOUNDARY_SHAPES)
def test_wave_and_block_boundaries(hip_engine, ploidy, A, C):
    """G' = 63, 64, 65; 55 and 66; the largest diploid event (G = 990) cut to 3 and to 946 genotypes and kept whole; ploidy
    1 023 over two alleles (G = G' = 1 024: every LDS row full).  Three samples, so three of the four waves work."""
    events = boundary_events(ploidy, A, C)
    res = check_exact(hip_engine, events, 3, ploidy, (ploidy, A, C))
    assert res.sub_pl[0].shape == (3, G.genotype_count(ploidy, C)) and res.sample_called.all()
    # ... and the posterior method over the same rows: log10_sum_log10 over more than one pass of the wave.  Every event is
    # compared: 2 % of the two drawn is none
    tally = {"drawn": 0, "skipped": 0, "max_deviation": 0.0}
    post = run(hip_engine, events, 3, ploidy, R.USE_POSTERIORS)
    for e, ev in enumerate(events):
        compare_posterior(post, e, want_of(ev, ploidy, R.USE_POSTERIORS), tally, (ploidy, A, C))
    print("boundary", (ploidy, A, C), tally)
    assert tally["drawn"] == 2 and tally["skipped"] <= MAX_SKIPPED * tally["drawn"], tally


def test_ties_go_to_the_lowest_index(hip_engine):
    """All PLs equal, and two equal minima in different lanes and different 64-wide chunks -- among them a pair whose higher
    index sits in the lower lane (65 is lane 1, 2 is lane 2)."""
    A, n = 13, G.genotype_count(2, 13)  # 91 genotypes: two passes of the wave
    rows = [[7] * n, [0] * n]
    for lo, hi in ((3, 67), (10, 75), (2, 65), (63, 64), (0, 90)):
        r = [40] * n
        r[lo] = r[hi] = 0
        rows.append(r)
        r = [40 + (i % 5) for i in range(n)]  # the second best tied as well: the `>=` scan's value
        r[hi], r[lo], r[(lo + 1) % n] = 0, 9, 9
        rows.append(r)
    ev = Event(*plain(A), list(range(A)), rows)
    res = check_exact(hip_engine, [ev], len(rows), 2)
    gts = R.G.genotypes(2, A)
    for k, (lo, hi) in enumerate(((3, 67), (10, 75), (2, 65), (63, 64), (0, 90))):
        al, cn = gts[lo]
        assert res.gt[0][2 + 2 * k].tolist() == [a for a, c in zip(al, cn) for _ in range(c)] and res.gq[0][2 + 2 * k] == 0
    assert res.gt[0][0].tolist() == [0, 0] and res.gq[0][0] == 0 and res.sample_called[0][0] == 1  # all equal, informative
    assert res.sample_flags[0][1] == R.UNINFORMATIVE


def test_uninformative_rows_and_the_threshold(hip_engine):
    """PLs [0, 1, 0] sum to -0.1, which is not below SUM_GL_THRESH_NOCALL: a no-call.  [0, 1, 1] is informative."""
    ev = Event(*plain(2), [0, 1], [[0, 0, 0], [0, 1, 0], [1, 0, 0], [0, 1, 1], [1, 1, 0], [0, 0, 2]])
    res = check_exact(hip_engine, [ev], 6, 2)
    assert res.sample_flags[0].tolist() == [R.UNINFORMATIVE] * 3 + [0] * 3
    assert res.sample_called[0].tolist() == [0, 0, 0, 1, 1, 1] and res.gq[0].tolist() == [-1, -1, -1, 1, 1, 0]
    assert res.gt[0][:3].tolist() == [[-1, -1]] * 3 and res.sub_pl[0][1].tolist() == [0, 1, 0]
    # the same through a subset, and over many genotypes: a single 1 among zeros
    n = G.genotype_count(2, 13)
    rows = [[0] * n, [0] * 50 + [1] + [0] * (n - 51), [0] * 50 + [1, 1] + [0] * (n - 52)]
    res = check_exact(hip_engine, [Event(*plain(13), list(range(13)), rows)], 3, 2)
    assert res.sample_flags[0].tolist() == [R.UNINFORMATIVE, R.UNINFORMATIVE, 0]


def test_saturated_pls(hip_engine):
    """i32::MAX is the PL of a -inf GL: it stays saturated through pl / -10.0 and gls_to_pls, and bounds GQ."""
    M = I32_MAX
    rows = [[0, M, M, M, M, M], [M, M, 0, M, M, M], [M, M, M, M, M, 0], [M] * 6, [M, M, M, M - 1, M, M], [5, M, M, 0, M, 3]]
    events = [Event(*plain(3), keep, rows) for keep in ([0, 1, 2], [0, 2], [0, 1])]
    res = check_exact(hip_engine, events, 6, 2)
    assert res.sub_pl[0][0].tolist() == [0] + [M] * 5 and int(res.gq[0][0]) == M
    assert res.sub_pl[1][1].tolist() == [0, 0, 0] and res.gq[1][1] == 0  # every kept genotype saturated: renormalised to 0


def test_renormalisation_after_subsetting_shows(hip_engine):
    """The best kept genotype has a non-zero old PL: the new PLs are shifted so that their minimum is 0."""
    ev = Event(*plain(3), [0, 1], [[50, 30, 80, 0, 20, 40], [90, 95, 70, 10, 0, 5]])
    res = check_exact(hip_engine, [ev], 2, 2)
    assert res.sub_pl[0].tolist() == [[20, 0, 50], [20, 25, 0]] and res.gt[0].tolist() == [[0, 1], [1, 1]] and res.gq[0].tolist() == [20, 20]


def test_non_ref_in_the_best_genotype(hip_engine):
    """PLs zeroed, GT a no-call, GQ still set; <NON_REF> outside the call or outside the best genotype changes nothing."""
    kinds = [R.PLAIN, R.PLAIN, R.NON_REF]
    rows = [[60, 60, 60, 0, 60, 25], [0, 60, 60, 40, 60, 60], [60, 60, 60, 60, 60, 0]]
    events = [Event([1, 1, 0], kinds, [0, 1, 2], rows), Event([1, 1, 0], kinds, [0, 2], rows), Event([1, 1, 0], kinds, [0, 1], rows)]
    res = check_exact(hip_engine, events, 3, 2)
    assert res.sample_flags[0].tolist() == [R.NON_REF_BEST, 0, R.NON_REF_BEST] and res.sample_flags[2].tolist() == [0, 0, 0]
    assert res.sub_pl[0][0].tolist() == [0] * 6 and res.gt[0][0].tolist() == [-1, -1] and res.gq[0][0] == 25
    assert res.sample_called[0].tolist() == [0, 1, 0] and res.sub_pl[0][1].tolist() == rows[1]
