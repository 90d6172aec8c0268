"""phmm_allele_frequency at the edges of its layout, against the restatement (tests/af_restatement.py) with the TOL / MARGIN
rule and skip accounting of tests/test_af_hip.py: every genotypes-per-lane class (K = 1 at S = 2 .. 64, K = 4, 8, 16) at 7 to
11 wave passes, on both sides of the switch to four waves; a call mixing every class and both modes against each event run
alone; many alleles; '*' and <NON_REF> at high allele indices; large ploidy; the PL rows real data produces; P(variant
present) and QUAL against mpmath; and genotype likelihoods -> allele frequency end to end."""
import concurrent.futures as cf
import math
import multiprocessing
import os

import numpy as np
import pytest

import af_restatement as R
import genotype_restatement as G
from lorikeet_amd import genotype, synthetic
import test_af_hip as TA
from test_af_hip import SEEN, _compare, _grid_events, _run
from test_af_restatement_precision import _pvp_gate, mp_log10_one_minus_pow10

pytestmark = pytest.mark.gpu
AF_BLOCK_PASSES = 8  # phmm_af_internal.hpp
PL_MAX = 2 ** 31 - 1  # the PL of a -inf GL (phmm_genotype_likelihoods)
MINE = {"max_deviation": 0.0, "compared": 0, "skipped": 0, "random_compared": 0, "random_skipped": 0, "max_present_mp": 0.0,
        "max_large_ploidy": 0.0, "max_over_gate": 0.0}


def _layout(G_, n_samples):
    """What phmm_af.cpp derives per event: genotypes per lane K, segment width S, samples per pass, passes."""
    K = 1 if G_ <= 64 else 4 if G_ <= 256 else 8 if G_ <= 512 else 16
    S = 64
    if K == 1:
        S = 1
        while S < G_:
            S <<= 1
    spp = 64 // S
    return K, S, spp, (n_samples + spp - 1) // spp


def _samples_for(G_, passes):
    """A sample count that takes `passes` wave passes, the last one partly filled where a pass holds several samples."""
    spp = _layout(G_, 1)[2]
    n = passes * spp - spp // 3
    assert _layout(G_, n)[3] == passes
    return n


@pytest.fixture(scope="module")
def pool():
    with cf.ProcessPoolExecutor(min(16, os.cpu_count() or 1), mp_context=multiprocessing.get_context("spawn")) as p:
        yield p


def _wants(pool, jobs):
    """jobs: [(events, ploidy, pseudo)] -> per job the restatement of each of its events, in a spawn process pool."""
    args = [[([(ploidy, list(map(int, s))) for s in pls], list(ln), list(kd), pseudo, 30.0)] for ev, ploidy, pseudo in jobs
            for ln, kd, pls in ev]
    flat = [w[0] for w in pool.map(R.calculate_many, args)]
    out, i = [], 0
    for ev, _, _ in jobs:
        out.append(flat[i:i + len(ev)])
        i += len(ev)
    return out


def _em_gate(ploidy, want):
    """The gate of an event.  TOL, except above ploidy 20 (beyond tests/test_af_hip.py's grid), where an EM that converges
    slowly is conditioned badly: there a count moves by a fraction rho < 1 of its last move per iteration (all-zero samples
    at ploidy 1 023: rho ~ 0.99 over hundreds of iterations), and a rounding difference of one iteration -- ocml's log10 and
    pow against libm's, times counts near the ploidy -- reaches the fixed point scaled by up to 1 / (1 - rho).  So the gate
    is TOL / (1 - rho), rho the largest ratio of successive count moves over the restatement's second half of iterations."""
    d = want.get("count_diffs", [])
    if ploidy <= 20 or len(d) < 3:
        return TA.TOL
    h = len(d) // 2
    rho = max(b / a for a, b in zip(d[h - 1:-1], d[h:]) if a > 0.0)
    return TA.TOL / max(1.0 - min(rho, 0.999), 1e-3)


def _cmp(res, e, want, fixed, ploidy=2):
    """_compare of tests/test_af_hip.py (its TOL replaced by _em_gate for large ploidy), with this file's own tally besides
    the shared one."""
    before, SEEN["max_deviation"] = dict(SEEN), 0.0
    tol, gate = TA.TOL, _em_gate(ploidy, want)
    TA.TOL = gate
    try:
        ok = _compare(res, e, want, fixed)
    finally:
        TA.TOL = tol
        dev = SEEN["max_deviation"]
        key = "max_deviation" if gate == tol else "max_large_ploidy"
        MINE[key] = max(MINE[key], dev)
        MINE["max_over_gate"] = max(MINE["max_over_gate"], dev / gate)
        SEEN["max_deviation"] = max(before["max_deviation"], dev)
    MINE["compared" if ok else "skipped"] += 1
    if not fixed:
        MINE["random_compared" if ok else "random_skipped"] += 1
    return ok


def _check_jobs(eng, pool, jobs, fixed=False):
    """Each job one call: (events, ploidy, pseudo) with the sample count its PLs carry."""
    results = []
    for (ev, ploidy, pseudo), wants in zip(jobs, _wants(pool, jobs)):
        res = _run(eng, ev, len(ev[0][2]), ploidy, pseudo)
        for e, w in enumerate(wants):
            _cmp(res, e, w, fixed, ploidy)
        results.append(res)
    return results


# ---- every class on both sides of the four-wave switch ------------------------------------------------------------------

CLASSES = [(1, 2), (2, 2), (2, 3), (2, 4), (2, 6), (2, 8), (2, 12), (2, 24), (2, 32)]  # (ploidy, A): G = 2, 3, 6, 10, 21, 36, 78, 300, 528


def test_every_class_at_7_to_11_passes(hip_engine, pool):
    seen = set()
    jobs = []
    rng = np.random.default_rng(31)
    for ploidy, A in CLASSES:
        g = G.genotype_count(ploidy, A)
        for passes in (7, 8, 9, 10, 11):
            n = _samples_for(g, passes)
            K, S = _layout(g, n)[:2]
            seen.add((K, S, passes >= AF_BLOCK_PASSES))
            pseudo = R.pseudo_counts() if passes % 2 else (1.0, 0.1, 0.05)
            jobs.append((_grid_events(rng, ploidy, A, n), ploidy, pseudo))
    assert {(k, s) for k, s, _ in seen} == {(1, 2), (1, 4), (1, 8), (1, 16), (1, 32), (1, 64), (4, 64), (8, 64), (16, 64)}
    assert all((k, s, b) in seen for k, s, _ in seen for b in (False, True))
    _check_jobs(hip_engine, pool, jobs)


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def test_mixed_call_equals_each_event_alone(hip_engine):
    """One call with events of every class, in one wave and in four (n_samples 40: K = 1 at S <= 8 one wave, the rest four;
    n_samples 7: every class one wave), shuffled: each event's results bit-identical to the event run alone."""
    rng = np.random.default_rng(41)
    for n_samples in (40, 7):
        ev = []
        for ploidy, A in CLASSES:
            if ploidy != 2:
                continue
            for _ in range(3):
                ev += _grid_events(rng, 2, A, n_samples)
        modes = {_layout(G.genotype_count(2, len(e[0])), n_samples)[3] >= AF_BLOCK_PASSES for e in ev}
        assert modes == ({False, True} if n_samples == 40 else {False})
        ev = [ev[i] for i in rng.permutation(len(ev))]
        whole = _run(hip_engine, ev, n_samples, 2, R.pseudo_counts())
        for e in range(len(ev)):
            one = _run(hip_engine, [ev[e]], n_samples, 2, R.pseudo_counts())
            for nm in ("log10_p_no_variant", "log10_p_variant_present", "qual", "flags", "iterations"):
                assert _same(getattr(one, nm)[:1], getattr(whole, nm)[e:e + 1]), (nm, e)
            for nm in ("log10_p_absent", "mle_count", "allele_flags"):
                assert _same(getattr(one, nm)[0], getattr(whole, nm)[e]), (nm, e)


# ---- many alleles, '*' and <NON_REF> at high indices, large ploidy ---------------------------------------------------

MANY = [(2, 7), (2, 16), (2, 31), (2, 32), (2, 33), (2, 44), (1, 7), (1, 33), (1, 49), (1, 50), (3, 17), (4, 10), (5, 8)]


def test_many_alleles(hip_engine, pool):
    rng = np.random.default_rng(43)
    jobs = [(_grid_events(rng, ploidy, A, n), ploidy, R.pseudo_counts()) for ploidy, A in MANY for n in (1, 9, 40)
            if n < 40 or G.genotype_count(ploidy, A) <= 136]  # (40 samples up to 16 alleles: the restatement's time)
    _check_jobs(hip_engine, pool, jobs)


def _span_del_event(rng, ploidy, A, sd, non_ref, n_samples):
    """'*' at allele sd, <NON_REF> last if asked; a third of the samples favour a genotype over {ref, '*'} alone."""
    g = G.genotype_count(ploidy, A)
    off = G.offset_table(ploidy, A)
    kinds = [R.PLAIN] * A
    kinds[sd] = R.SPAN_DEL
    if non_ref:
        kinds[-1] = R.NON_REF
    pls = rng.integers(20, 3000, size=(n_samples, g))
    for s in range(n_samples):
        n_sd = int(rng.integers(0, ploidy + 1))
        best = G.alleles_to_index([0] * (ploidy - n_sd) + [sd] * n_sd, off) if s % 3 == 0 else int(rng.integers(0, g))
        pls[s, best] = 0
    length = [1] + [0 if k == R.NON_REF else int(rng.choice([1, 2])) for k in kinds[1:]]
    return length, kinds, pls


def test_span_del_and_non_ref_at_high_indices(hip_engine, pool):
    rng = np.random.default_rng(47)
    jobs = []
    for ploidy, A, sd, non_ref in ((2, 44, 1, True), (2, 44, 31, True), (2, 44, 32, True), (2, 44, 33, True), (2, 44, 43, False),
                                   (1, 50, 31, True), (1, 50, 32, True), (1, 50, 43, True), (2, 34, 33, False)):
        for n in (3, 9):
            jobs.append(([_span_del_event(rng, ploidy, A, sd, non_ref, n)], ploidy, R.pseudo_counts()))
    _check_jobs(hip_engine, pool, jobs)


@pytest.mark.parametrize("ploidy,A", [(21, 2), (63, 2), (64, 2), (100, 2), (255, 2), (511, 2), (1023, 2), (43, 3)])
def test_large_ploidy(hip_engine, pool, ploidy, A):
    rng = np.random.default_rng(ploidy)
    jobs = [(_grid_events(rng, ploidy, A, n), ploidy, R.pseudo_counts()) for n in (1, 3, 9)]
    _check_jobs(hip_engine, pool, jobs)


# ---- the PL rows real data produces ------------------------------------------------------------------------------------

def test_zero_rows_and_saturated_pls(hip_engine, pool):
    rng = np.random.default_rng(53)
    jobs = []
    for ploidy, A in ((2, 2), (2, 3), (2, 12), (2, 32), (100, 2), (1023, 2), (1, 50)):
        g = G.genotype_count(ploidy, A)
        for n in (1, 5, 9):
            pls = rng.integers(0, 400, size=(n, g))
            pls[np.arange(n), rng.integers(0, g, size=n)] = 0
            pls[0] = 0                                          # a sample without coverage: a G-way tie
            if n > 1:
                pls[1, rng.random(g) < 0.5] = PL_MAX            # -inf GLs
                pls[1, 0] = 0
            if n > 2:
                pls[2] = PL_MAX                                 # one finite genotype
                pls[2, int(rng.integers(0, g))] = 0
            jobs.append(([([1] * A, [R.PLAIN] * A, pls)], ploidy, R.pseudo_counts()))
            if ploidy <= 100:  # every sample empty (at ploidy 1 023 the restatement's EM takes thousands of iterations)
                jobs.append(([([1] * A, [R.PLAIN] * A, np.zeros((n, g), np.int64))], ploidy, R.pseudo_counts()))
    _check_jobs(hip_engine, pool, jobs)


# ---- P(variant present) and QUAL against mpmath -------------------------------------------------------------------------

def test_variant_present_against_mpmath(hip_engine):
    """log10(1 - 10^pnv) of the device's own P(no variant), at 50 digits: pnv from about -1e-15 to about -300, across the
    log1mexp branch threshold log(0.5).  Gate: 1e-13 relative plus the reference formula's own conditioning (_pvp_gate)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    ev = []
    for h in np.unique(np.round(np.logspace(0, math.log10(3100), 120)).astype(int)):
        ev.append(([1, 1], [R.PLAIN] * 2, [[0, int(h), int(2 * h)]]))  # hom-ref favoured: pnv from about -0.3 up to 0
        ev.append(([1, 1], [R.PLAIN] * 2, [[int(h), 0, int(2 * h)]]))  # het favoured: pnv down to about -h / 10
    for n in range(1, 40):  # the region of the threshold, finely
        ev.append(([1, 1], [R.PLAIN] * 2, [[n, 0, 3 * n]]))
    res = _run(hip_engine, ev, 1, 2, R.pseudo_counts())
    pnv = res.log10_p_no_variant
    t = R.LOG1MEXP_THRESHOLD / R.LOG_10
    nz = pnv[pnv < 0.0]
    assert nz.min() < -250.0 and nz.max() > -1e-14 and np.sum(nz < t) > 20 and np.sum((nz > t) & (nz < -1e-3)) > 10
    for e in range(len(ev)):
        x = float(pnv[e])
        got, qual = float(res.log10_p_variant_present[e]), float(res.qual[e])
        if x == 0.0:
            assert got == -math.inf
            continue
        want = mp_log10_one_minus_pow10(mp, x)
        rel = float(abs((got - want) / want))
        MINE["max_present_mp"] = max(MINE["max_present_mp"], rel)
        assert rel <= _pvp_gate(x), (x, got, rel)
        want_qual = -10 * want if res.flags[e] & R.MONOMORPHIC else -10 * mp.mpf(x)
        assert float(abs((qual - want_qual) / want_qual)) <= _pvp_gate(x), (x, qual)


# ---- end to end: genotype likelihoods -> allele frequency -------------------------------------------------------------

@pytest.mark.parametrize("ploidy,A,n_haps,n_reads", [(2, 16, 20, 60), (1023, 2, 4, 150)])
def test_end_to_end(hip_engine, ploidy, A, n_haps, n_reads):
    import test_genotype_hip as TG
    rng = np.random.default_rng(ploidy + A)
    batch = synthetic.make_regions(1, n_reads, n_haps, 100, [50, 70], seed=ploidy)
    L = hip_engine.compute(batch)
    n_samples = 3
    sample = rng.integers(0, n_samples, size=n_reads).astype(np.uint32)
    start = rng.integers(0, 60, size=n_reads).astype(np.int64)
    end = start + rng.integers(0, 50, size=n_reads)
    hap = np.concatenate([rng.permutation(A), rng.integers(-1, A, size=n_haps - A)]).astype(np.int32)
    ev = genotype.Events([0, 0], [0, A, 2 * A], [40, 50], [44, 54], np.concatenate([hap, rng.permutation(hap)]))
    gt = TG._check(hip_engine, batch, L, None, sample, start, end, ev, ploidy, n_samples)  # bit-equal to the restatement
    assert int(gt.n_evidence.sum()) > 0
    res = genotype.allele_frequency(hip_engine, gt, allele_off=ev.allele_off, allele_length=np.ones(2 * A, np.uint32), ploidy=ploidy,
                                    pseudo_counts=R.pseudo_counts(), stand_min_conf=30.0)
    want_gt = G.batch_events(batch, L, None, sample, start, end, n_samples, ploidy, ev)
    for e in range(ev.n_events):
        want = R.calculate_genotypes([(ploidy, list(map(int, s))) for s in want_gt[e][1]], [1] * A, [R.PLAIN] * A,
                                     R.pseudo_counts(), 30.0)
        _cmp(res, e, want, False, ploidy)


def test_report():
    print("\nphmm_allele_frequency edges vs restatement: %d events compared, %d skipped (%d of %d random), largest relative "
          "deviation %.3g up to ploidy 20, %.3g above (largest deviation / gate %.3g); log10_p_variant_present vs mpmath: "
          "largest relative deviation %.3g" %
          (MINE["compared"], MINE["skipped"], MINE["random_skipped"], MINE["random_compared"] + MINE["random_skipped"],
           MINE["max_deviation"], MINE["max_large_ploidy"], MINE["max_over_gate"], MINE["max_present_mp"]))
    n_random = MINE["random_compared"] + MINE["random_skipped"]
    assert MINE["random_skipped"] == 0 or MINE["random_skipped"] < 0.01 * n_random
