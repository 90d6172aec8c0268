"""phmm_assign_genotypes on the MI355X against the restatement of the reference's genotype assignment
(tests/assign_restatement.py).

The default method (UsePLsToAssign) is integers and single IEEE operations: sub_pl, gt, gq, sample_called and the flags must
equal the restatement integer for integer, log10_gq bit for bit.  The posterior method's gt, sample_called and flags are
exact; gp, pg, log10_gq and log10_p_error_posterior must lie within tests/af_restatement.py's gate, 1e-11 x max(1, |want|)
(ocml pow / log10 against libm), and gq must be equal for every case whose decisions -- the gap between the two largest
posteriors, the distance of -10 log10 GQ from a half -- are at least 1e-9 (relative) from their boundary.  Cases nearer are
left out and counted: at most 2 % of those drawn (tests/test_assign_oracle.py checks the seeds on the CPU)."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import assign_restatement as R
import genotype_restatement as G
from lorikeet_amd import _lib, genotype
from lorikeet_amd.engine import PhmmError

pytestmark = pytest.mark.gpu
TOL, MARGIN, MAX_SKIPPED = 1e-11, 1e-9, 0.02
SNP_HET, INDEL_HET = -3.0, math.log10(1.25e-4)
_i32p = C.POINTER(C.c_int32)


class Event:
    """One event of a call: lengths / kinds of its alleles, keep = the call's alleles, pls [n_samples][G], monomorphic."""

    def __init__(self, lengths, kinds, keep, pls, mono=0):
        self.lengths, self.kinds, self.keep, self.mono = list(lengths), list(kinds), list(keep), int(mono)
        self.pls = [list(map(int, s)) for s in pls]


def plain(A):
    return [1] * A, [R.PLAIN] * A


def run(eng, events, S, ploidy, method=R.USE_PLS):
    a_off = np.concatenate([[0], np.cumsum([len(e.lengths) for e in events])]).astype(np.uint32)
    pls = [np.asarray(e.pls, np.int32).reshape(-1) for e in events]
    pl_off = np.concatenate([[0], np.cumsum([len(p) for p in pls])]).astype(np.uint64)
    return genotype.assign_genotypes(eng, [e.keep for e in events], np.concatenate(pls), a_off, pl_off,
                                     np.concatenate([e.lengths for e in events]), np.concatenate([e.kinds for e in events]),
                                     n_samples=S, ploidy=ploidy, method=method, log10_snp_het=SNP_HET, log10_indel_het=INDEL_HET,
                                     site_monomorphic=[e.mono for e in events])


def want_of(ev, ploidy, method=R.USE_PLS):
    return R.assign_event(ploidy, ev.lengths, ev.kinds, ev.keep, ev.pls, method, SNP_HET, INDEL_HET, bool(ev.mono))


def same_f64(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def compare_exact(res, e, w, tag=None):
    """Everything the default method writes for event e against assign_event's dict."""
    tag = (tag, e)
    assert [list(r) for r in res.sub_pl[e]] == w["sub_pl"] or (not any(w["sub_pl"]) and res.sub_pl[e].size == 0), ("sub_pl", tag)
    assert res.gt[e].tolist() == w["gt"], ("gt", tag, res.gt[e].tolist(), w["gt"])
    assert res.gq[e].tolist() == w["gq"], ("gq", tag, res.gq[e].tolist(), w["gq"])
    assert same_f64(res.log10_gq[e], w["log10_gq"]), ("log10_gq", tag, res.log10_gq[e], w["log10_gq"])
    assert res.sample_called[e].tolist() == w["called"], ("called", tag)
    assert res.sample_flags[e].tolist() == w["flags"], ("flags", tag, res.sample_flags[e].tolist(), w["flags"])


def check_exact(eng, events, S, ploidy, tag=None):
    res = run(eng, events, S, ploidy)
    for e, ev in enumerate(events):
        compare_exact(res, e, want_of(ev, ploidy), tag)
    return res


def dev(got, want):
    if math.isinf(want) or math.isinf(got) or math.isnan(want) or math.isnan(got):
        assert got == want or (math.isnan(got) and math.isnan(want)), (got, want)
        return 0.0
    return abs(got - want) / max(1.0, abs(want))


def compare_posterior(res, e, w, tally, tag=None):
    """Event e of a posterior-method result; False when the restatement reports a decision within MARGIN of its boundary."""
    tag = (tag, e)
    tally["drawn"] += 1
    if w["margin"] < MARGIN:
        tally["skipped"] += 1
        return False
    assert res.gt[e].tolist() == w["gt"], ("gt", tag, res.gt[e].tolist(), w["gt"])
    assert res.sample_called[e].tolist() == w["called"] and res.sample_flags[e].tolist() == w["flags"], ("called / flags", tag)
    assert [list(r) for r in res.sub_pl[e]] == w["sub_pl"] or res.sub_pl[e].size == 0, ("sub_pl", tag)
    d = [dev(g, x) for g, x in zip(res.log10_gq[e], w["log10_gq"])] + [dev(float(res.log10_p_error_posterior[e]), w["qual_update"])]
    if w["gp"] is not None:
        d += [dev(g, x) for got, want in ((res.gp[e], w["gp"]), (res.pg[e], w["pg"])) for gr, wr in zip(got, want) for g, x in zip(gr, wr)]
    tally["max_deviation"] = max(tally["max_deviation"], max(d))
    print("posterior", tag, "max deviation %.3g" % max(d), "margin %.3g" % w["margin"])
    assert max(d) <= TOL, (tag, max(d))
    assert res.gq[e].tolist() == w["gq"], ("gq", tag, res.gq[e].tolist(), w["gq"])
    return True


def random_pls(rng, S, n, hi=120):
    """PL rows as the genotyping step writes them: non-negative with a zero."""
    pls = rng.integers(0, hi, size=(S, n))
    pls[np.arange(S), rng.integers(0, n, size=S)] = 0
    return pls


def subsets_with_ref(A):
    return [[0] + list(c) for k in range(A) for c in itertools.combinations(range(1, A), k)]


def grid_events(rng, ploidy, S):
    """A_e = 2 .. 6 with every subset that contains the reference (the identity and C_e == 1 among them); the last allele is
    <NON_REF> in every third event."""
    events = []
    for A in range(2, 7):
        n = G.genotype_count(ploidy, A)
        for i, keep in enumerate(subsets_with_ref(A)):
            kinds = [R.PLAIN] * (A - 1) + [R.NON_REF if i % 3 == 0 else R.PLAIN]
            events.append(Event([1] * A, kinds, keep, random_pls(rng, S, n)))
    return events


# ---- the default method -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ploidy", [1, 2, 3, 5])
def test_default_method_grid_is_exact(hip_engine, ploidy):
    for S in (1, 2, 3):
        events = grid_events(np.random.default_rng(1000 * ploidy + S), ploidy, S)
        res = check_exact(hip_engine, events, S, ploidy, (ploidy, S))
        flags = np.concatenate([f.reshape(-1) for f in res.sample_flags])
        assert (flags & R.REF_ONLY).any() and (flags & R.NON_REF_BEST).any() and (res.gt >= 1).any()


def test_sample_called_is_the_type_predicate(hip_engine):
    """Het, HomVar and HomRef are called; the uninformative and the <NON_REF> no-calls are not."""
    ln, kd = plain(3)
    rows = [[0, 30, 60, 30, 60, 60], [30, 0, 60, 30, 60, 60], [60, 30, 0, 60, 60, 60], [0, 0, 0, 0, 0, 0], [60, 60, 60, 30, 60, 0]]
    ev = Event(ln, [R.PLAIN, R.PLAIN, R.NON_REF], [0, 1, 2], rows)
    res = check_exact(hip_engine, [ev], 5, 2)
    assert res.sample_called[0].tolist() == [1, 1, 1, 0, 0]
    assert res.gt[0].tolist() == [[0, 0], [0, 1], [1, 1], [-1, -1], [-1, -1]]
    assert res.sample_flags[0].tolist() == [0, 0, 0, R.UNINFORMATIVE, R.NON_REF_BEST]
    assert res.gq[0].tolist() == [30, 30, 30, -1, 30] and res.sub_pl[0][4].tolist() == [0] * 6


def test_mixed_call_equals_each_event_alone(hip_engine):
    rng = np.random.default_rng(5)
    for method in (R.USE_PLS, R.USE_POSTERIORS):
        events = []
        for A, keep in ((2, [0, 1]), (6, [0, 2, 5]), (4, []), (3, [0]), (44, [0, 7, 43]), (5, [0, 1, 2, 3, 4]), (2, [])):
            events.append(Event([1, 2, 1, 3, 1, 1][:A] + [1] * max(0, A - 6), [R.PLAIN] * A, keep,
                                random_pls(rng, 5, G.genotype_count(2, A), 3000), mono=A % 2))
        whole = run(hip_engine, events, 5, 2, method)
        for e, ev in enumerate(events):
            one = run(hip_engine, [ev], 5, 2, method)
            assert np.array_equal(whole.sub_pl[e], one.sub_pl[0]) and np.array_equal(whole.gt[e], one.gt[0])
            assert np.array_equal(whole.gq[e], one.gq[0]) and same_f64(whole.log10_gq[e], one.log10_gq[0])
            assert np.array_equal(whole.sample_called[e], one.sample_called[0]) and np.array_equal(whole.sample_flags[e], one.sample_flags[0])
            if method == R.USE_POSTERIORS:
                assert same_f64(whole.gp[e], one.gp[0]) and same_f64(whole.pg[e], one.pg[0])
                assert same_f64(whole.log10_p_error_posterior[e:e + 1], one.log10_p_error_posterior[:1])


def test_empty_call_list_gives_zeroed_outputs(hip_engine):
    rng = np.random.default_rng(6)
    events = [Event(*plain(3), [], random_pls(rng, 2, 6)), Event(*plain(2), [0, 1], random_pls(rng, 2, 3)), Event(*plain(4), [], random_pls(rng, 2, 10))]
    for method in (R.USE_PLS, R.USE_POSTERIORS):
        res = run(hip_engine, events, 2, 2, method)
        for e in (0, 2):
            assert res.sub_pl[e].size == 0 and not res.gt[e].any() and not res.gq[e].any() and not res.log10_gq[e].any()
            assert not res.sample_called[e].any() and not res.sample_flags[e].any()
            if method == R.USE_POSTERIORS:
                assert res.gp[e].size == 0 and res.log10_p_error_posterior[e] == 0.0
        assert res.sample_called[1].all()


# ---- the posterior method ---------------------------------------------------------------------------------------------------

def posterior_events(seed):
    """SNP, indel and '*' alleles at ploidy 1, 2, 3 and 5, both arms of the QUAL update: [(ploidy, S, events)]."""
    rng = np.random.default_rng(seed)
    out = []
    for ploidy in (1, 2, 3, 5):
        for S in (1, 2, 3):
            events = []
            for A in range(2, 6):
                n = G.genotype_count(ploidy, A)
                for keep in subsets_with_ref(A):
                    lengths = [2] + [int(x) for x in rng.choice([2, 2, 1, 5], size=A - 1)]
                    kinds = [R.PLAIN] * A
                    if A > 2 and rng.random() < 0.4:
                        star = int(rng.integers(1, A))
                        kinds[star], lengths[star] = R.SPAN_DEL, 1
                    hi = int(rng.choice([40, 300, 4000]))  # posteriors a few units apart: every term of the log sums counts
                    events.append(Event(lengths, kinds, keep, random_pls(rng, S, n, hi), mono=int(rng.random() < 0.5)))
            out.append((ploidy, S, events))
    return out


POSTERIOR_SEED = 20


def test_posterior_method_grid(hip_engine):
    tally = {"drawn": 0, "skipped": 0, "max_deviation": 0.0}
    arms = set()
    for ploidy, S, events in posterior_events(POSTERIOR_SEED):
        res = run(hip_engine, events, S, ploidy, R.USE_POSTERIORS)
        for e, ev in enumerate(events):
            if compare_posterior(res, e, want_of(ev, ploidy, R.USE_POSTERIORS), tally, (ploidy, S)) and len(ev.keep) > 1:
                arms.add((ev.mono, R.SPAN_DEL in [ev.kinds[a] for a in ev.keep]))
    print("posterior grid:", tally)
    assert tally["skipped"] <= MAX_SKIPPED * tally["drawn"], tally
    assert arms == {(0, False), (0, True), (1, False), (1, True)}


def test_posterior_gq_arms(hip_engine):
    """get_gq_log10_from_posteriors: two and three genotypes, and the general arm with the best first, last and inside."""
    tally = {"drawn": 0, "skipped": 0, "max_deviation": 0.0}
    cases = [(1, 2, [[0, 35], [35, 0]]), (1, 3, [[0, 31, 47], [31, 0, 47], [47, 31, 0]]), (2, 2, [[0, 31, 47], [31, 0, 47], [47, 31, 0]]),
             (1, 5, [[0, 33, 41, 52, 67], [67, 52, 41, 33, 0], [41, 33, 0, 52, 67]]),
             (2, 3, [[0, 33, 41, 52, 67, 71], [67, 52, 41, 33, 71, 0], [41, 33, 0, 52, 67, 71]])]
    for ploidy, A, rows in cases:
        ev = Event([1] * A, [R.PLAIN] * A, list(range(A)), [[10 * x + 3 for x in r] for r in rows])
        ev.pls = [[x - min(r) for x in r] for r in ev.pls]
        res = run(hip_engine, [ev], len(rows), ploidy, R.USE_POSTERIORS)
        assert compare_posterior(res, 0, want_of(ev, ploidy, R.USE_POSTERIORS), tally, (ploidy, A))


# ---- the chain ---------------------------------------------------------------------------------------------------------------

def test_end_to_end_chain_without_a_host_step(hip_engine):
    """phmm_genotype_likelihoods -> phmm_allele_frequency -> phmm_assign_genotypes -> phmm_annotate_events with the device's
    sample_called equals the chain with sample_called from the restatement."""
    from test_genotype_hip import _random_case
    rng = np.random.default_rng(31)
    S = 3
    b, L, keep, sample, start, end, ev = _random_case(rng, 2, [2, 3, 4, 3, 2, 5], S, n_reads=30)
    gl = genotype.genotype_likelihoods(hip_engine, b, L, keep, start, end, sample, ev, ploidy=2, n_samples=S)
    lengths = np.ones(int(ev.allele_off[-1]), np.uint32)
    af = genotype.allele_frequency(hip_engine, gl, allele_off=ev.allele_off, allele_length=lengths, stand_min_conf=5.0)
    res = genotype.assign_genotypes(hip_engine, af, gl, allele_off=ev.allele_off, allele_length=lengths)
    calls = genotype.call_alleles_of(af)
    assert res.call_alleles == calls and sum(1 for c in calls if len(c) >= 2) >= 1
    called = np.zeros((ev.n_events, S), np.uint8)
    for e in range(ev.n_events):
        w = R.assign_event(2, [1] * ev.n_alleles(e), [R.PLAIN] * ev.n_alleles(e), calls[e], gl.pl[e].tolist())
        compare_exact(res, e, w)
        called[e] = w["called"]
    mapq = np.full(b.n_reads, 60, np.uint8)
    err = af.qual / -10.0
    got = genotype.annotate_events(hip_engine, b, L, keep, start, end, sample, mapq, ev, calls, err, n_samples=S, sample_called=res)
    ref = genotype.annotate_events(hip_engine, b, L, keep, start, end, sample, mapq, ev, calls, err, n_samples=S, sample_called=called)
    for name in ("dp", "ac", "info_dp", "qd_depth", "flags"):
        assert np.array_equal(getattr(got, name), getattr(ref, name)), name
    assert same_f64(got.qd, ref.qd) and all(np.array_equal(a, c) for a, c in zip(got.ad, ref.ad))


# ---- refused arguments ----------------------------------------------------------------------------------------------------------

_NAMES = ["event_allele_off", "allele_length", "allele_kind", "pl_off", "pl", "call_allele_off", "call_allele", "site_monomorphic",
          "sub_pl_off", "sub_pl", "gt", "gq", "log10_gq", "sample_called", "sample_flags", "gp", "pg", "log10_p_error_posterior"]
_TYPES = dict(allele_kind=np.uint8, pl_off=np.uint64, pl=np.int32, site_monomorphic=np.uint8, sub_pl_off=np.uint64, sub_pl=np.int32,
              gt=np.int32, gq=np.int32, log10_gq=np.float64, sample_called=np.uint8, sample_flags=np.uint8, gp=np.float64,
              pg=np.float64, log10_p_error_posterior=np.float64)
_CT = {np.uint8: _lib.u8p, np.uint32: _lib.u32p, np.uint64: _lib.u64p, np.int32: _i32p, np.float64: _lib.f64p}
_OUTPUTS = ["sub_pl", "gt", "gq", "log10_gq", "sample_called", "sample_flags", "gp", "pg", "log10_p_error_posterior"]


def _raw(eng, n_events, n_samples, ploidy, method, a):
    p = {k: None if a.get(k) is None else np.ascontiguousarray(a[k], _TYPES.get(k, np.uint32)).ctypes.data_as(_CT[_TYPES.get(k, np.uint32)])
         for k in _NAMES}
    return eng.lib.phmm_assign_genotypes(eng._h, n_events, n_samples, ploidy, p["event_allele_off"], p["allele_length"], p["allele_kind"],
                                         p["pl_off"], p["pl"], p["call_allele_off"], p["call_allele"], method, SNP_HET, INDEL_HET,
                                         p["site_monomorphic"], p["sub_pl_off"], p["sub_pl"], p["gt"], p["gq"], p["log10_gq"],
                                         p["sample_called"], p["sample_flags"], p["gp"], p["pg"], p["log10_p_error_posterior"])


def test_invalid_arguments_write_nothing(hip_engine):
    eng = hip_engine

    def good():  # two diploid events of one sample: A = 2 with the call {0, 1}, A = 3 with the call {0, 2}
        return dict(event_allele_off=[0, 2, 5], allele_length=[1, 1, 1, 1, 2], allele_kind=[0, 0, 0, 0, 0], pl_off=[0, 3, 9],
                    pl=[0, 20, 40, 50, 10, 0, 40, 30, 60], call_allele_off=[0, 2, 4], call_allele=[0, 1, 0, 2], site_monomorphic=[0, 1],
                    sub_pl_off=[0, 3, 6])

    def run_(n_events=2, n_samples=1, ploidy=2, method=R.USE_POSTERIORS, **change):
        a = good()
        a.update(change)
        outs = dict(sub_pl=np.full(8, 7, np.int32), gt=np.full(8, 7, np.int32), gq=np.full(4, 7, np.int32), log10_gq=np.full(4, 7.5),
                    sample_called=np.full(4, 7, np.uint8), sample_flags=np.full(4, 7, np.uint8), gp=np.full(8, 7.5), pg=np.full(8, 7.5),
                    log10_p_error_posterior=np.full(4, 7.5))
        for k in _OUTPUTS:
            a[k] = None if (k in change and change[k] is None) else outs[k]
        code = _raw(eng, n_events, n_samples, ploidy, method, a)
        return code, all(np.all(v == (7.5 if v.dtype == np.float64 else 7)) for v in outs.values()), outs

    code, untouched, outs = run_()
    assert code == _lib.PHMM_OK and not untouched, eng.last_error()
    assert outs["gt"][:4].tolist() == [0, 0, 0, 0] and outs["sub_pl"][:6].tolist() == [0, 20, 40, 10, 0, 20]  # (the indel prior)
    code, untouched, outs = run_(method=R.USE_PLS, allele_length=None, gp=None, pg=None, log10_p_error_posterior=None, log10_gq=None,
                                 site_monomorphic=None, allele_kind=None)
    assert code == _lib.PHMM_OK and outs["gq"][:2].tolist() == [20, 10] and outs["sample_called"][:2].tolist() == [1, 1]
    assert outs["gt"][:4].tolist() == [0, 0, 0, 1] and outs["sub_pl"][:6].tolist() == [0, 20, 40, 10, 0, 20]
    bad = {
        "unknown method": dict(method=2),
        "ploidy must be": dict(ploidy=0),
        "event_allele_off not monotonic": dict(event_allele_off=[0, 2, 1]),
        "pl_off not monotonic": dict(pl_off=[0, 3, 2]),
        "call_allele_off not monotonic": dict(call_allele_off=[0, 2, 1]),
        "sub_pl_off not monotonic": dict(sub_pl_off=[0, 3, 2]),
        "event 1: fewer than 2 alleles": dict(event_allele_off=[0, 2, 3]),
        "event 1: 1035 genotypes": dict(event_allele_off=[0, 2, 47]),
        "call_allele[0] is not 0": dict(call_allele=[0, 1, 1, 2]),
        "event 1: call allele 1 outside": dict(call_allele=[0, 1, 0, 3]),
        "not strictly increasing": dict(call_allele_off=[0, 1, 4], call_allele=[0, 0, 2, 2]),
        "pl_off slot smaller": dict(pl_off=[0, 3, 8]),
        "sub_pl_off slot smaller": dict(sub_pl_off=[0, 3, 5]),
        "unknown kind": dict(allele_kind=[0, 0, 0, 0, 3]),
        "cannot take <NON_REF>": dict(allele_kind=[0, 0, 0, 0, 2]),
    }
    for name in ("event_allele_off", "pl_off", "call_allele_off", "call_allele", "sub_pl_off", "gt", "gq", "sample_called", "sample_flags",
                 "pl", "sub_pl", "allele_length", "gp", "pg", "log10_p_error_posterior"):
        bad["null array|" + name] = {name: None}
    for what, change in bad.items():
        code, untouched, _ = run_(**change)
        assert code == _lib.PHMM_ERR_INVALID_ARG and untouched, (what, code, eng.last_error())
        assert eng.last_error().startswith("phmm_assign_genotypes") and what.split("|")[0] in eng.last_error(), (what, eng.last_error())
    code, untouched, _ = run_(n_events=0)
    assert code == _lib.PHMM_OK and untouched
    # <NON_REF> in the call is the default method's business
    code, untouched, outs = run_(method=R.USE_PLS, allele_kind=[0, 0, 0, 0, 2])
    assert code == _lib.PHMM_OK and outs["gt"][:4].tolist() == [0, 0, -1, -1] and outs["sample_flags"][1] == R.NON_REF_BEST
    with pytest.raises(PhmmError):
        genotype.assign_genotypes(eng, [[0, 2]], [0, 1, 2], [0, 2], [0, 3], [1, 1])
