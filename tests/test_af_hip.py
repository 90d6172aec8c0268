"""phmm_allele_frequency on the MI355X against the restatement of the reference's allele-frequency step
(tests/af_restatement.py): the reference's own test cases at uniform ploidy, a random-PL grid over ploidy x alleles x
samples, '*' and <NON_REF> events, the 50-allele cutoff, the whole path from a region call, the activity-profile shape,
batch invariance and run-to-run determinism, and every refused argument.

Log10 outputs and QUAL must lie within 1e-11 x max(1, |want|) of the restatement; counts, iterations and flags must be equal
unless the restatement reports a decision quantity within 1e-9 (relative) of its boundary -- such random events are skipped
and counted (fewer than 1 %), fixed cases must be clear of it."""
import concurrent.futures as cf
import ctypes as C
import math
import multiprocessing
import os

import numpy as np
import pytest

import af_restatement as R
import genotype_restatement as G
from lorikeet_amd import _lib, genotype, synthetic
from lorikeet_amd.engine import PhmmError

pytestmark = pytest.mark.gpu
TOL, MARGIN = 1e-11, 1e-9
SEEN = {"max_deviation": 0.0, "compared": 0, "skipped": 0}


def _flat(events):
    """events: [(allele_length, allele_kind, pls [n_samples][G])] -> the call's flat arrays."""
    a_off = np.concatenate([[0], np.cumsum([len(e[0]) for e in events])]).astype(np.uint32)
    pls = [np.asarray(e[2], np.int32).reshape(-1) for e in events]
    pl_off = np.concatenate([[0], np.cumsum([len(p) for p in pls])]).astype(np.uint64)
    length = np.concatenate([e[0] for e in events]).astype(np.uint32)
    kind = np.concatenate([e[1] for e in events]).astype(np.uint8)
    return a_off, length, kind, pl_off, np.concatenate(pls) if pls else np.zeros(0, np.int32)


def _run(eng, events, n_samples, ploidy, pseudo, smc=30.0):
    a_off, length, kind, pl_off, pl = _flat(events)
    return genotype.allele_frequency(eng, pl, pl_off, a_off, length, kind, n_samples, ploidy, pseudo, smc)


def _dev(got, want):
    if math.isinf(want) or math.isinf(got) or math.isnan(want):
        assert got == want or (math.isnan(got) and math.isnan(want)), (got, want)
        return 0.0
    return abs(got - want) / max(1.0, abs(want))


def _compare(res, e, want, fixed=True):
    """One event of a device result against calculate_genotypes' dict; returns False when it was skipped."""
    if want["margin"] < MARGIN:
        assert not fixed, ("a fixed case sits on a decision boundary", want["margin"])
        SEEN["skipped"] += 1
        return False
    SEEN["compared"] += 1
    assert int(res.flags[e]) == want["flags"], (e, res.flags[e], want["flags"])
    if want["flags"] & R.TOO_MANY_ALLELES or "log10_p_no_variant" not in want:
        return True
    # log10_p_variant_present = log10(1 - 10^pnv) magnifies an absolute error of pnv by 1 / |pnv ln 10|: where pnv is near 0
    # one ulp of pnv's sum moves it far beyond the gate.  So it (and QUAL when it comes from it) is held to the restatement's
    # function of the device's own pnv; pnv itself is held to the gate, and the raw deviation is reported apart.
    pnv = float(res.log10_p_no_variant[e])
    pvp = R.log10_one_minus_pow10(pnv)
    qual = (-10.0 * (pvp + 0.0 if want["flags"] & R.MONOMORPHIC else pnv + 0.0)) + 0.0
    d = [_dev(pnv, want["log10_p_no_variant"]), _dev(res.log10_p_variant_present[e], pvp), _dev(res.qual[e], qual),
         _dev(res.qual[e], want["qual"]) if not want["flags"] & R.MONOMORPHIC else 0.0] + \
        [_dev(g, w) for g, w in zip(res.log10_p_absent[e][1:], want["log10_p_absent"][1:])]
    SEEN["max_deviation"] = max(SEEN["max_deviation"], max(d))
    SEEN["max_raw_present"] = max(SEEN.get("max_raw_present", 0.0), _dev(res.log10_p_variant_present[e], want["log10_p_variant_present"]))
    assert max(d) <= TOL, (e, d)
    assert res.log10_p_absent[e][0] == 0.0
    assert list(res.mle_count[e]) == want["mle"], (e, list(res.mle_count[e]), want["mle"])
    assert int(res.iterations[e]) == want["iterations"]
    assert list(res.allele_flags[e]) == want["allele_flags"]
    return True


def _check(eng, events, n_samples, ploidy, pseudo, smc=30.0, fixed=True, wants=None):
    res = _run(eng, events, n_samples, ploidy, pseudo, smc)
    if wants is None:
        wants = [R.calculate_genotypes([(ploidy, list(map(int, s))) for s in pls], list(ln), list(kd), pseudo, smc)
                 for ln, kd, pls in events]
    for e, w in enumerate(wants):
        _compare(res, e, w, fixed)
    return res


def obvious(ploidy, n_alleles, counts, pl):
    alleles = [a for a, c in zip(counts[::2], counts[1::2]) for _ in range(c)]
    out = [pl] * G.genotype_count(ploidy, n_alleles)
    out[G.alleles_to_index(alleles, G.offset_table(ploidy, n_alleles))] = 0
    return out


def _plain(A):
    return [1] * A, [R.PLAIN] * A


# ---- the reference's test cases (allele_frequency_calculator_unit_tests.rs) at uniform ploidy ----------------------------

def test_reference_cases_on_device(hip_engine):
    f, x = 20, 1000
    AA, BB, CC = obvious(2, 3, [0, 2], f), obvious(2, 3, [1, 2], f), obvious(2, 3, [2, 2], f)
    AB, AC = obvious(2, 3, [0, 1, 1, 1], f), obvious(2, 3, [0, 1, 2, 1], f)
    ln, kd = _plain(3)
    # symmetries and MLE counts: diploid sites of 2 and 3 samples
    for n, sets in ((2, [[AA, BB], [AA, CC], [AA, AB], [AA, AC], [AB, AB], [AC, AC]]),
                    (3, [[AA, AA, BB], [AA, AA, CC], [AA, AB, AB], [AA, AC, AC], [AA, AB, AC]])):
        for pseudo in ((1.0, 0.1, 0.1), (1.0, 1.0, 1.0)):
            res = _check(hip_engine, [(ln, kd, s) for s in sets], n, 2, pseudo)
            if pseudo == (1.0, 0.1, 0.1) and n == 2:
                for a, b in ((0, 1), (2, 3), (4, 5)):
                    assert abs(res.log10_p_no_variant[a] - res.log10_p_no_variant[b]) <= 1e-3
                    assert abs(res.log10_p_absent[a][1] - res.log10_p_absent[b][2]) <= 1e-3
            if pseudo == (1.0, 1.0, 1.0):
                want = {2: [[2, 0], [0, 2], [1, 0], [0, 1], [2, 0], [0, 2]], 3: [[2, 0], [0, 2], [2, 0], [0, 2], [1, 1]]}[n]
                assert [list(m[1:]) for m in res.mle_count] == want
    # many samples with low confidence: counts 0, 0, 2, >= 3 at 1, 2, 5, 9 samples
    ab2 = obvious(2, 2, [0, 1, 1, 1], f)
    got = [int(_check(hip_engine, [(*_plain(2), [ab2] * n)], n, 2, (1000.0, 1.0, 1.0)).mle_count[0][1]) for n in (1, 2, 5, 9)]
    assert got[:3] == [0, 0, 2] and got[3] >= 3
    # 100 and 1 000 very confident samples
    acx = obvious(2, 3, [0, 1, 2, 1], x)
    for n in (100, 1000):
        r = _check(hip_engine, [(ln, kd, [acx] * n)], n, 2, (1.0, 1.0, 1.0))
        assert list(r.mle_count[0][1:]) == [0, n]
        assert abs(r.log10_p_absent[0][2] - n * (math.log10(0.5) - x / 10.0)) <= n * 0.01
    # approximate multiplicative confidence
    aa3, bb3 = AA[:3], BB[:3]
    p = [_check(hip_engine, [(*_plain(2), [aa3, bb3] * (i + 1))], 2 * (i + 1), 2, (1.0, 1.0, 1.0)).log10_p_no_variant[0] for i in range(10)]
    assert all(abs((p[i + 1] - p[i]) - p[0]) <= 0.01 for i in range(9))
    # reference samples do not kill a good variant (the restatement up to 10 000 samples; the assertion alone at 100 000)
    aax, abx = obvious(2, 2, [0, 2], x), obvious(2, 2, [0, 1, 1, 1], x)
    for n_ref in (1, 10, 100, 1000, 10000, 100000):
        ev = [(*_plain(2), [aax] * n_ref + [abx])]
        r = _check(hip_engine, ev, n_ref + 1, 2, (1.0, 0.1, 0.1)) if n_ref <= 10000 else _run(hip_engine, ev, n_ref + 1, 2, (1.0, 0.1, 0.1))
        assert r.log10_p_no_variant[0] < -x / 10.0 + math.log10(n_ref) + 1.0
    # spanning deletions (uniform ploidy)
    sd3 = ([1, 1, 1], [R.PLAIN, R.PLAIN, R.SPAN_DEL])
    span_del, low_qual_snp = [50, 100, 100, 0, 100, 100], [10, 0, 40, 100, 70, 300]
    r1 = _check(hip_engine, [(*sd3, [span_del]), (*sd3, [low_qual_snp])], 1, 2, (1.0, 0.1, 0.1))
    r2 = _check(hip_engine, [(*sd3, [low_qual_snp, span_del])], 2, 2, (1.0, 0.1, 0.1))
    assert r1.log10_p_variant_present[0] < -10.0
    assert abs(r1.log10_p_variant_present[1] - r2.log10_p_variant_present[0]) <= 0.1
    assert r2.log10_p_variant_present[0] < r1.log10_p_variant_present[1]
    r3 = _check(hip_engine, [(*_plain(2), [[50, 0, 50]]), (*sd3, [[50, 0, 50, 100, 100, 100]])], 1, 2, (1.0, 0.1, 0.1))
    assert abs(r3.log10_p_variant_present[0] - r3.log10_p_variant_present[1]) <= 1e-4
    r4 = _check(hip_engine, [([1, 1, 1], [R.PLAIN, R.SPAN_DEL, R.PLAIN], [[0] + [10000] * 14])], 1, 4, (1.0, 0.1, 0.1))
    assert r4.log10_p_no_variant[0] <= 0.0


# ---- random PLs over ploidy x alleles x samples -----------------------------------------------------------------------

def _grid_events(rng, ploidy, A, n_samples):
    g = G.genotype_count(ploidy, A)
    pls = rng.integers(0, 100000, size=(n_samples, g))
    pls[rng.random(pls.shape) < 0.5] //= 1000                      # most PLs small
    pls[np.arange(n_samples), rng.integers(0, g, size=n_samples)] = 0  # a best genotype per sample
    pls[rng.random(pls.shape) < 0.1] = 0                            # ties at 0
    if g > 2:
        pls[:, 1] = pls[:, 2]                                       # ties elsewhere
    length = [1] + [int(v) for v in rng.choice([1, 1, 2, 0], size=A - 1)]
    return [(length, [R.PLAIN] * A, pls.astype(np.int32))]


def test_random_grid(hip_engine):
    rng = np.random.default_rng(2026)
    jobs = []
    for ploidy in range(1, 21):
        for A in range(2, 7):
            if G.genotype_count(ploidy, A) > 1024:
                continue
            for n_samples in (1, 3, 64):
                pseudo = R.pseudo_counts() if rng.random() < 0.5 else (1.0, 0.1, 0.05)
                jobs.append((ploidy, n_samples, pseudo, _grid_events(rng, ploidy, A, n_samples)))
    cases = [[(ploidy, list(map(int, s))) for s in ev[0][2]] for ploidy, _, _, ev in jobs]
    args = [[(c, ev[0][0], ev[0][1], pseudo, 30.0)] for c, (_, _, pseudo, ev) in zip(cases, jobs)]
    with cf.ProcessPoolExecutor(min(16, os.cpu_count() or 1), mp_context=multiprocessing.get_context("spawn")) as pool:
        wants = [w[0] for w in pool.map(R.calculate_many, args)]
    before = dict(SEEN)
    for (ploidy, n_samples, pseudo, ev), want in zip(jobs, wants):
        _check(hip_engine, ev, n_samples, ploidy, pseudo, fixed=False, wants=[want])
    compared, skipped = SEEN["compared"] - before["compared"], SEEN["skipped"] - before["skipped"]
    print("\nrandom grid: %d events compared, %d skipped at a boundary, largest deviation %.3g" %
          (compared, skipped, SEEN["max_deviation"]))
    assert skipped < 0.01 * (compared + skipped)


# ---- '*' and <NON_REF>, the cutoffs -----------------------------------------------------------------------------------

def test_span_del_and_non_ref_events(hip_engine):
    rng = np.random.default_rng(5)
    events = []
    for kinds in ([0, 2], [0, 1], [0, 1, 0], [0, 0, 1], [0, 0, 2], [0, 2, 0, 1], [0, 1, 2]):
        for ploidy_pls in range(3):
            g = G.genotype_count(2, len(kinds))
            pls = rng.integers(0, 300, size=(3, g))
            pls[:, ploidy_pls % g] = 0
            events.append(([1] + [0 if k == 2 else 1 for k in kinds[1:]], kinds, pls))
    # the lone <NON_REF> is output even when implausible, and makes the site called
    events.append(([1, 0], [0, 2], np.array([[0, 300, 300]] * 3)))
    res = _check(hip_engine, events, 3, 2, R.pseudo_counts())
    last = len(events) - 1
    assert res.allele_flags[last][1] == _lib.PHMM_AF_ALLELE_OUTPUT and res.called(last)
    sd = [e for e, ev in enumerate(events) if 1 in ev[1]]
    assert all(not (res.allele_flags[e][list(events[e][1]).index(1)] & _lib.PHMM_AF_ALLELE_OUTPUT) for e in sd)


def test_allele_cutoff_and_no_samples(hip_engine):
    ev = [([1] * 50, [0] * 50, np.arange(50)[None, :] * 7), ([1] * 51, [0] * 51, np.zeros((1, 51)))]
    res = _check(hip_engine, ev, 1, 1, R.pseudo_counts())
    assert not res.flags[0] & _lib.PHMM_AF_TOO_MANY_ALLELES and res.flags[1] == _lib.PHMM_AF_TOO_MANY_ALLELES
    empty = _run(hip_engine, [([1, 1], [0, 0], np.zeros((0, 3))), ([1] * 51, [0] * 51, np.zeros((0, 51)))], 0, 2, R.pseudo_counts())
    assert list(empty.flags) == [0, _lib.PHMM_AF_TOO_MANY_ALLELES] and list(empty.qual) == [0.0, 0.0]


# ---- end to end, the activity profile, batch invariance ---------------------------------------------------------------

def test_end_to_end_from_the_region_call(hip_engine):
    import test_genotype_hip as TG
    batch = synthetic.make_regions(6, 40, 4, 120, [50, 70], seed=77)
    one, ref_start = TG._region_call(hip_engine, batch, 77)
    orig_start = np.repeat(ref_start, np.diff(batch.region_read_off.astype(np.int64)))
    start = np.where(one.reads.status == 0, one.reads.new_pos, orig_start).astype(np.int64)
    end = start + 49
    ev = synthetic.make_events(batch, region_reference_start=ref_start)
    sample = (np.arange(batch.n_reads) % 3).astype(np.uint32)
    for ploidy in (1, 2, 3):
        gt = genotype.genotype_likelihoods(hip_engine, batch, one.likelihoods, one.keep.astype(np.uint8), start, end, sample, ev,
                                           ploidy=ploidy, n_samples=3)
        length = np.ones(int(ev.allele_off[-1]), np.uint32)
        res = genotype.allele_frequency(hip_engine, gt, allele_off=ev.allele_off, allele_length=length, ploidy=ploidy,
                                        pseudo_counts=R.pseudo_counts(), stand_min_conf=30.0)
        for e in range(ev.n_events):
            want = R.calculate_genotypes([(ploidy, list(map(int, s))) for s in gt.pl[e]], [1] * ev.n_alleles(e), [0] * ev.n_alleles(e),
                                         R.pseudo_counts(), 30.0)
            _compare(res, e, want, fixed=False)
        assert res.flags.any()


def _activity(rng, n, n_samples=16):
    """N / <FAKE_ALT> at ploidy 2: per sample the PLs of (ref, het, hom-alt) from ref-vs-any likelihoods."""
    ev = []
    for _ in range(n):
        het = rng.random(n_samples) < 0.1
        pls = np.stack([np.where(het, rng.integers(10, 400, n_samples), 0), np.where(het, 0, rng.integers(3, 60, n_samples)),
                        rng.integers(20, 800, n_samples)], axis=1)
        ev.append(([1, 0], [0, 0], pls))
    return ev


def test_activity_profile_shape(hip_engine):
    rng = np.random.default_rng(9)
    ev = _activity(rng, 400)
    res = _check(hip_engine, ev, 16, 2, R.pseudo_counts(), fixed=False)
    assert (res.flags & _lib.PHMM_AF_CALLED).any() and not (res.flags & _lib.PHMM_AF_CALLED).all()


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def test_batch_invariance_and_determinism(hip_engine):
    rng = np.random.default_rng(13)
    ev = []
    for e in range(4096):  # wave events of every genotype class, and four-wave events (many samples at G <= 64 and beyond)
        ploidy_shape = [(2, 2), (2, 3), (2, 5), (4, 4), (2, 12), (2, 30)][e % 6]
        A = ploidy_shape[1]
        g = G.genotype_count(2, A)
        ev.append(([1] * A, [0] * A, rng.integers(0, 200, size=(40, g))))
    whole = _run(hip_engine, ev, 40, 2, R.pseudo_counts())
    again = _run(hip_engine, ev, 40, 2, R.pseudo_counts())
    names = ("log10_p_no_variant", "log10_p_variant_present", "qual", "flags", "iterations")
    for nm in names:
        assert _same(getattr(whole, nm), getattr(again, nm)), nm
    for lo, hi in ((0, 1), (1, 700), (700, 701), (701, 4096)):
        part = _run(hip_engine, ev[lo:hi], 40, 2, R.pseudo_counts())
        for nm in names:
            assert _same(getattr(part, nm), getattr(whole, nm)[lo:hi]), (nm, lo)
        for nm in ("log10_p_absent", "mle_count", "allele_flags"):
            for k in range(hi - lo):
                assert _same(getattr(part, nm)[k], getattr(whole, nm)[lo + k]), (nm, lo + k)
    some = list(range(0, 4096, 257))
    _check(hip_engine, [ev[e] for e in some], 40, 2, R.pseudo_counts(), fixed=False)


# ---- refused arguments --------------------------------------------------------------------------------------------------

def test_invalid_arguments_write_nothing(hip_engine):
    lib = hip_engine.lib
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731

    def call(a_off, length, kind, pl_off, pl, ploidy=2, n_samples=1, null=None):
        n = len(a_off) - 1
        na = int(max(a_off)) if len(a_off) else 0
        outs = dict(pnv=np.full(n, 7.0), pvp=np.full(n, 7.0), absent=np.full(na, 7.0), mle=np.full(na, 7, np.int64),
                    af=np.full(na, 7, np.uint8), qual=np.full(n, 7.0), flags=np.full(n, 7, np.uint32), it=np.full(n, 7, np.uint32))
        args = [p(np.asarray(a_off, np.uint32), _lib.u32p), p(np.asarray(length, np.uint32), _lib.u32p),
                p(None if kind is None else np.asarray(kind, np.uint8), _lib.u8p), p(np.asarray(pl_off, np.uint64), _lib.u64p),
                p(np.asarray(pl, np.int32), i32p)]
        outp = [p(outs["pnv"], _lib.f64p), p(outs["pvp"], _lib.f64p), p(outs["absent"], _lib.f64p), p(outs["mle"], i64p),
                p(outs["af"], _lib.u8p), p(outs["qual"], _lib.f64p), p(outs["flags"], _lib.u32p), p(outs["it"], _lib.u32p)]
        if null is not None:
            full = args + outp
            full[null] = None
            args, outp = full[:5], full[5:]
        code = lib.phmm_allele_frequency(hip_engine._h, n, n_samples, ploidy, *args[:5], 10.0, 0.01, 0.00125, 30.0, *outp)
        untouched = all(np.all(v == 7) for v in outs.values())
        return code, untouched

    good = ([0, 2, 4], [1, 1, 1, 1], [0, 0, 0, 0], [0, 3, 6], [0, 10, 20, 5, 0, 9])
    code, _ = call(*good)
    assert code == _lib.PHMM_OK
    bad = [
        dict(args=([0, 2, 1], [1, 1, 1], None, [0, 3, 6], [0] * 6), why="event_allele_off not monotonic"),
        dict(args=([0, 2, 4], [1] * 4, None, [0, 6, 3], [0] * 6), why="pl_off not monotonic"),
        dict(args=([0, 2, 3], [1] * 3, None, [0, 3, 6], [0] * 6), why="fewer than 2 alleles"),
        dict(args=([0, 2, 4], [1] * 4, [0, 0, 1, 0], [0, 3, 6], [0] * 6), why="allele 0 (the reference) is not plain"),
        dict(args=([0, 3], [1] * 3, [0, 1, 1], [0, 6], [0] * 6), why="more than one '*' allele"),
        dict(args=([0, 2, 4], [1] * 4, [0, 3, 0, 0], [0, 3, 6], [0] * 6), why="unknown kind"),
        dict(args=([0, 2, 4], [1] * 4, None, [0, 3, 5], [0] * 6), why="pl_off slot smaller"),
        dict(args=([0, 45], [1] * 45, None, [0, 1035], [0] * 1035), why="more than 1024"),
        dict(args=good, kw=dict(ploidy=0), why="ploidy must be at least 1"),
    ]
    for b in bad:
        code, untouched = call(*b["args"], **b.get("kw", {}))
        assert code == _lib.PHMM_ERR_INVALID_ARG and untouched, b["why"]
        assert b["why"] in hip_engine.last_error(), (b["why"], hip_engine.last_error())
    for null in (0, 1, 3, 4, 5, 6, 7, 8, 10, 11):  # every required array (allele_kind, allele_flags and iterations may be NULL)
        code, untouched = call(*good, null=null)
        assert code == _lib.PHMM_ERR_INVALID_ARG and untouched, null
    assert lib.phmm_allele_frequency(hip_engine._h, 0, 1, 2, *([None] * 5), 1.0, 1.0, 1.0, 30.0, *([None] * 8)) == _lib.PHMM_OK
    with pytest.raises(PhmmError):
        genotype.allele_frequency(hip_engine, np.zeros(6, np.int32), [0, 3, 6], [0, 2, 3], [1, 1, 1], None, 1, 2)


def test_report():
    print("\nphmm_allele_frequency vs restatement: %d events compared, %d skipped, largest relative deviation %.3g "
          "(log10_p_variant_present against the restatement's own: %.3g)" %
          (SEEN["compared"], SEEN["skipped"], SEEN["max_deviation"], SEEN.get("max_raw_present", 0.0)))
