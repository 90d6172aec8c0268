"""phmm_genotype_likelihoods on the MI355X: GLs, PLs and evidence counts bit-equal to the restatement of the reference's
genotyping step (tests/genotype_restatement.py), for random matrices over ploidy x allele count, the edge cases of the
read predicate and the PL conversion, the whole per-region path end to end, large batches, long events, and every
refused argument."""
import ctypes as C

import numpy as np
import pytest

import genotype_restatement as R
from lorikeet_amd import _lib, genotype, region, synthetic
from lorikeet_amd.engine import PhmmError
from oracle import oracle

pytestmark = pytest.mark.gpu
_i32p, _i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


class _Batch:
    """The region layout phmm_genotype_likelihoods reads (reads x haplotypes per region, matrices back to back)."""

    def __init__(self, reads, haps, gap=0):
        self.n_regions = len(reads)
        self.region_read_off = np.concatenate([[0], np.cumsum(reads)]).astype(np.uint32)
        self.region_hap_off = np.concatenate([[0], np.cumsum(haps)]).astype(np.uint32)
        sizes = np.asarray(reads, np.int64) * np.asarray(haps, np.int64) + gap
        self.out_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        self.n_reads = int(self.region_read_off[-1])


def _same(got, want):
    return got.shape == want.shape and np.array_equal(np.asarray(got).view(np.uint8), np.asarray(want).view(np.uint8))


def _check(eng, b, L, keep, sample, start, end, ev, ploidy, n_samples, only=None):
    res = genotype.genotype_likelihoods(eng, b, L, keep, start, end, sample, ev, ploidy=ploidy, n_samples=n_samples)
    want = R.batch_events(b, L, keep, sample, start, end, n_samples, ploidy, ev, only=only)
    for e, (gl, pl, ne) in want.items():
        assert _same(res.gl[e], gl), ("GL", e, ev.n_alleles(e), res.gl[e], gl)
        assert np.array_equal(res.pl[e], pl), ("PL", e, res.pl[e], pl)
        assert np.array_equal(res.n_evidence[e], ne), ("n_evidence", e)
    return res


def _random_case(rng, ploidy, alleles, n_samples, n_reads=24, n_haps=6, span=60):
    """One region per allele count, each with one event: random likelihoods with -inf entries, all -inf rows, exact
    ties and zeros; keep = 0 reads; a sample without reads (the last, when there are several); reads of every overlap kind."""
    nr, nh = [], []
    L, keep, sample, start, end = [], [], [], [], []
    region, a_off, w0, w1, maps = [], [0], [], [], []
    for g, A in enumerate(alleles):
        r, h = n_reads + int(rng.integers(0, 8)), n_haps + int(rng.integers(0, 4))
        m = -np.abs(rng.normal(0.0, 2.0, size=(r, h)))
        m[rng.random((r, h)) < 0.08] = -np.inf
        m[rng.integers(0, r)] = -np.inf
        m[:, 1] = m[:, 0]  # exact ties between haplotypes
        m[rng.random((r, h)) < 0.05] = 0.0
        m = np.round(m * 4) / 4 if rng.random() < 0.3 else m  # ties between alleles too
        L.append(m.reshape(-1))
        keep.append((rng.random(r) > 0.1).astype(np.uint8))
        sample.append(rng.integers(0, max(1, n_samples - 1), size=r) if n_samples > 1 else np.zeros(r, np.int64))
        s = rng.integers(0, span, size=r)
        ln = rng.integers(0, 25, size=r)
        ln[rng.random(r) < 0.1] = 0  # a read that consumes no reference base: end == start
        start.append(s)
        end.append(s + np.maximum(ln - 1, 0))
        mp = rng.integers(-1, A, size=h)
        if A > 1 and rng.random() < 0.3:
            mp[mp == A - 1] = 0  # an allele no haplotype maps to
        maps.append(mp)
        c = int(rng.integers(5, span - 5))
        region.append(g)
        a_off.append(a_off[-1] + A)
        w0.append(c - 2)
        w1.append(c + 2)
        nr.append(r)
        nh.append(h)
    b = _Batch(nr, nh)
    ev = genotype.Events(region, a_off, w0, w1, np.concatenate(maps))
    return b, np.concatenate(L), np.concatenate(keep), np.concatenate(sample).astype(np.uint32), \
        np.concatenate(start).astype(np.int64), np.concatenate(end).astype(np.int64), ev


def _alleles_for(ploidy):
    every = [a for a in range(1, 1025) if R.genotype_count(ploidy, a) <= 1024]
    return every if len(every) <= 48 else [1, 2, 3, 4, 5, 8, 17, 33, 100, 512, 1024]


@pytest.mark.parametrize("ploidy", [1, 2, 3, 4, 20])
@pytest.mark.parametrize("n_samples", [1, 3])
def test_random_matrices_bit_equal(hip_engine, ploidy, n_samples):
    for seed in (1, 2):
        rng = np.random.default_rng(seed * 1000 + ploidy * 10 + n_samples)
        case = _random_case(rng, ploidy, _alleles_for(ploidy), n_samples)
        res = _check(hip_engine, *case, ploidy, n_samples)
        if n_samples == 3:
            assert all(int(res.n_evidence[e][2]) == 0 for e in range(case[-1].n_events))  # the sample without reads


def test_overlap_clauses_and_pl_edges(hip_engine):
    # window [10, 14]; reads: start inside, end inside, enclosing, inside, zero-length at the edges, outside either side
    start = np.array([12, 5, 3, 11, 10, 14, 15, 0, 9, 12], np.int64)
    end = np.array([30, 10, 40, 13, 10, 14, 20, 9, 9, 12], np.int64)
    used = R.overlaps(10, 14, start, end)
    assert list(used) == [True, True, True, True, True, True, False, False, False, True]
    n = len(start)
    rng = np.random.default_rng(5)
    L = -np.abs(rng.normal(0, 1, size=(n, 3)))
    b = _Batch([n, n, n], [3, 3, 3])
    # event 0: ordinary; event 1: every haplotype unmapped (all GLs -inf -> PLs 0); event 2: allele 1 unmapped (-inf next to finite)
    ev = genotype.Events([0, 1, 2], [0, 2, 4, 6], [10, 10, 10], [14, 14, 14], [0, 1, 1, -1, -1, -1, 0, 0, -1])
    keep = np.ones(3 * n, np.uint8)
    keep[3] = 0
    res = _check(hip_engine, b, np.tile(L.reshape(-1), 3), keep, np.zeros(3 * n, np.uint32), np.tile(start, 3), np.tile(end, 3), ev, 2, 1)
    assert list(res.n_evidence[:, 0]) == [6, 7, 7]
    assert np.all(res.gl[1] == -np.inf) and np.all(res.pl[1] == 0)
    assert res.pl[2][0, 2] == 2 ** 31 - 1 and res.pl[2][0, 0] == 0 and res.gl[2][0, 2] == -np.inf and np.isfinite(res.gl[2][0, 1])


def _region_call(eng, batch, seed):
    cfg = _lib.EngineConfig()
    cfg.constant_gcp, cfg.pcr_error_model, cfg.base_quality_score_threshold = 10, 3, 18
    cfg.symmetrically_normalize_alleles_to_reference, cfg.log10_global_read_mismapping_rate = 1, -4.5
    cfg.read_disqualification_scale, cfg.expected_error_rate_per_base = 1.0, 0.02
    n, G = batch.n_reads, batch.n_regions
    H = int(batch.hap_off[1] - batch.hap_off[0])
    hap_cigars = [oracle.parse_cigar("%dM" % H)] * batch.n_haps
    orig = [oracle.parse_cigar("%dM" % (batch.read_off[r + 1] - batch.read_off[r])) for r in range(n)]
    ref_start = [1000 + 7000 * g for g in range(G)]
    one = region.region_compute(eng, cfg, batch, np.full(n, 60, np.uint8), hap_cigars, [0] * batch.n_haps, [0] * G, ref_start, orig)
    return one, ref_start


def test_end_to_end_from_the_region_call(hip_engine):
    batch = synthetic.make_regions(6, 40, 4, 120, [50, 70], seed=77)
    one, ref_start = _region_call(hip_engine, batch, 77)
    assert np.all(one.reads.status >= 0) and np.mean(one.reads.status == 0) > 0.9
    # a realigned read is where the projection put it; one the reference leaves as it is (status 1: no informative best
    # allele) keeps its original alignment -- here at its region's start with its original CIGAR
    orig_start = np.repeat(ref_start, np.diff(batch.region_read_off.astype(np.int64)))
    moved = one.reads.status == 0
    start = np.where(moved, one.reads.new_pos, orig_start).astype(np.int64)
    cigars = [c if m else oracle.parse_cigar("%dM" % (batch.read_off[r + 1] - batch.read_off[r]))
              for r, (c, m) in enumerate(zip(one.reads.cigars, moved))]
    end = np.array([genotype.read_end(p, c) for p, c in zip(start, cigars)], np.int64)
    ev = synthetic.make_events(batch, region_reference_start=ref_start)
    assert ev.n_events >= 6
    sample = (np.arange(batch.n_reads) % 2).astype(np.uint32)
    for ploidy in (2, 3):
        res = _check(hip_engine, batch, one.likelihoods, one.keep.astype(np.uint8), sample, start, end, ev, ploidy, 2)
        assert int(res.n_evidence.sum()) > 0


def test_batch_invariance(hip_engine):
    rng = np.random.default_rng(11)
    G = 2000
    nr, nh = rng.integers(4, 24, size=G), rng.integers(2, 5, size=G)
    b = _Batch(nr, nh)
    L = -np.abs(rng.normal(0, 2, size=int(b.out_off[-1])))
    n = b.n_reads
    sample, keep = rng.integers(0, 2, size=n).astype(np.uint32), (rng.random(n) > 0.05).astype(np.uint8)
    start = rng.integers(0, 100, size=n).astype(np.int64)
    end = start + rng.integers(0, 60, size=n)
    region, a_off, w, maps = [], [0], [], []
    for g in range(G):
        for _ in range(int(rng.integers(3, 6))):
            A = int(rng.integers(2, 4))
            region.append(g)
            a_off.append(a_off[-1] + A)
            w.append(int(rng.integers(0, 150)))
            maps.append(rng.integers(-1, A, size=int(nh[g])))
    ev = genotype.Events(region, a_off, np.array(w) - 2, np.array(w) + 2, np.concatenate(maps))
    whole = _check(hip_engine, b, L, keep, sample, start, end, ev, 2, 2, only=list(range(0, ev.n_events, 97)))
    region_arr = np.asarray(region)
    moff = np.concatenate([[0], np.cumsum(nh[region_arr])])
    for g in range(0, G):
        es = np.flatnonzero(region_arr == g)
        r0, r1 = int(b.region_read_off[g]), int(b.region_read_off[g + 1])
        b1 = _Batch([nr[g]], [nh[g]])
        lo = int(b.out_off[g])
        e1 = genotype.Events(np.zeros(len(es)), np.concatenate([[0], np.cumsum(np.diff(ev.allele_off)[es])]), ev.start[es], ev.end[es],
                             np.concatenate([ev.hap_allele[moff[e]:moff[e + 1]] for e in es]))
        part = genotype.genotype_likelihoods(hip_engine, b1, L[lo:lo + int(nr[g] * nh[g])], keep[r0:r1], start[r0:r1], end[r0:r1],
                                             sample[r0:r1], e1, ploidy=2, n_samples=2)
        for k, e in enumerate(es):
            assert _same(part.gl[k], whole.gl[e]) and np.array_equal(part.pl[k], whole.pl[e])
            assert np.array_equal(part.n_evidence[k], whole.n_evidence[e])


def test_long_event_and_many_genotypes(hip_engine):
    rng = np.random.default_rng(3)
    # 5 000 reads: twenty tiles of the kernel; p = 3, A = 17: 969 genotypes (tiles of four reads)
    for n, nh, ploidy, A in ((5000, 4, 2, 3), (300, 20, 3, 17)):
        b = _Batch([n], [nh])
        L = -np.abs(rng.normal(0, 2, size=n * nh))
        start = rng.integers(0, 50, size=n).astype(np.int64)
        ev = genotype.Events([0], [0, A], [20], [24], rng.integers(0, A, size=nh))
        res = _check(hip_engine, b, L, None, np.zeros(n, np.uint32), start, start + 30, ev, ploidy, 1)
        assert res.gl[0].shape == (1, genotype.genotype_count(ploidy, A))


def _raw(eng, b, L, keep, sample, start, end, n_samples, ploidy, ev, gl_off, gl, pl, ne, n_events=None):
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)  # noqa: E731
    return eng.lib.phmm_genotype_likelihoods(
        eng._h, b.n_regions, p(b.region_read_off, _lib.u32p), p(b.region_hap_off, _lib.u32p), p(b.out_off, _lib.u64p), p(L, _lib.f64p),
        p(keep, _lib.u8p), p(sample, _lib.u32p), p(start, _i64p), p(end, _i64p), n_samples, ploidy,
        ev.n_events if n_events is None else n_events, p(ev.region, _lib.u32p), p(ev.allele_off, _lib.u32p), p(ev.start, _i64p),
        p(ev.end, _i64p), p(ev.hap_allele, _i32p), p(gl_off, _lib.u64p), p(gl, _lib.f64p), p(pl, _i32p), p(ne, _lib.u32p))


def test_invalid_arguments_write_nothing(hip_engine):
    eng = hip_engine
    b = _Batch([4, 3], [2, 3])
    L = -np.abs(np.random.default_rng(0).normal(size=int(b.out_off[-1])))
    sample, start, end = np.zeros(7, np.uint32), np.zeros(7, np.int64), np.full(7, 10, np.int64)

    def ev_(region=(0, 1), a_off=(0, 2, 4), hap=(0, 1, 0, 1, -1)):
        return genotype.Events(region, a_off, [0, 0], [5, 5], hap)

    def run(ev, ploidy=2, n_samples=1, gl_off=None, smp=sample, batch=b, null=None):
        G = [genotype.genotype_count(ploidy, ev.n_alleles(e)) for e in range(ev.n_events)]
        off = np.concatenate([[0], np.cumsum(np.array(G, np.uint64) * n_samples)]).astype(np.uint64) if gl_off is None else gl_off
        gl, pl, ne = np.full(64, 7.5), np.full(64, 7, np.int32), np.full(8, 7, np.uint32)
        args = [eng, batch, L, None, smp, start, end, n_samples, ploidy, ev, off, gl, pl, ne]
        if null is not None:
            args[null] = None
        code = _raw(*args)
        return code, gl, pl, ne

    code, gl, pl, ne = run(ev_())
    assert code == _lib.PHMM_OK and gl[0] != 7.5
    bad = {
        "null likelihoods": dict(null=2), "null gl": dict(null=11), "ploidy 0": dict(ploidy=0),
        "too many genotypes": dict(ev=ev_(a_off=(0, 2, 47))),  # 45 alleles, diploid: 1 035 genotypes
        "no alleles": dict(ev=ev_(a_off=(0, 0, 2))), "map below -1": dict(ev=ev_(hap=(0, -2, 0, 1, 1))),
        "map beyond A": dict(ev=ev_(hap=(0, 2, 0, 1, 1))), "event_region": dict(ev=ev_(region=(0, 2))),
        "offsets not monotonic": dict(ev=ev_(a_off=(0, 2, 1))),
        "read_sample": dict(smp=np.array([0, 0, 0, 1, 0, 0, 0], np.uint32)),
        "gl_off slot": dict(gl_off=np.array([0, 3, 5], np.uint64)),
        "region offsets": dict(batch=type("B", (), dict(n_regions=2, region_read_off=np.array([0, 4, 3], np.uint32),
                                                       region_hap_off=b.region_hap_off, out_off=b.out_off))()),
    }
    for what, kw in bad.items():
        code, gl, pl, ne = run(**{"ev": ev_(), **kw})
        assert code == _lib.PHMM_ERR_INVALID_ARG, what
        assert np.all(gl == 7.5) and np.all(pl == 7) and np.all(ne == 7), what
        assert eng.last_error().startswith("phmm_genotype_likelihoods"), what
    code, gl, pl, ne = run(genotype.Events([], [0], [], [], []))
    assert code == _lib.PHMM_OK and np.all(gl == 7.5)
    msg = None
    try:
        genotype.genotype_likelihoods(eng, b, L, None, start, end, sample, ev_(hap=(0, 1, 0, 5, 1)), ploidy=2)
    except PhmmError as e:
        msg = str(e)
    assert msg and "event 1" in msg
