"""phmm_genotype_likelihoods at the edges of its layout, bit-equal to the restatement (tests/genotype_restatement.py): the
genotype accumulators each lane keeps (g = t + 256 k: G = 256/257, 512/513, 768/769, 1 024), the read tiles through LDS
(T = min(256, 32 KB / (8 (A + G))) reads, used counts T - 1, T, T + 1 and 2T + 1 with and without dropped reads between
them), many alleles at low ploidy, many samples, and both sides of the ploidy and genotype-count limits."""
import numpy as np
import pytest

import genotype_restatement as R
from lorikeet_amd import _lib, genotype
from test_genotype_hip import _Batch, _check, _random_case, _raw

pytestmark = pytest.mark.gpu
GT_THREADS, GT_MAX_TILE, GT_LDS_BYTES = 256, 256, 32 * 1024  # phmm_genotype_internal.hpp
W0, W1 = 20, 24  # the event window of the cases built here


def _tile(A, G):
    """The kernel's tile: reads per pass through LDS."""
    return min(GT_MAX_TILE, GT_LDS_BYTES // (8 * (A + G)))


def _hap_map(rng, A, n_haps, unmapped=None):
    """Every allele on some haplotype (unless `unmapped`), the rest random, a few haplotypes on no allele (-1)."""
    mp = np.concatenate([rng.permutation(A), rng.integers(-1, A, size=n_haps - A)])
    mp[rng.random(n_haps) < 0.1] = -1
    if unmapped is not None:
        mp[mp == unmapped] = -1
    return rng.permutation(mp).astype(np.int32)


def _reads(rng, kinds):
    """A read per kind, in this order: 'use' (sample 0, kept, overlapping the window by one of the three clauses), 'keep'
    (dropped by keep), 'sample' (another sample's), 'outside' (next to the window, not on it)."""
    n = len(kinds)
    keep, sample = np.ones(n, np.uint8), np.zeros(n, np.uint32)
    start, end = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i, k in enumerate(kinds):
        c = int(rng.integers(0, 3))
        start[i], end[i] = [(W0 + 2, W0 + 30), (W0 - 9, W0 + 1), (W0 - 12, W1 + 12)][c]
        if k == "keep":
            keep[i] = 0
        elif k == "sample":
            sample[i] = 1
        elif k == "outside":
            start[i], end[i] = [(W1 + 1, W1 + 40), (0, W0 - 1)][c % 2]
    assert list(R.overlaps(W0, W1, start, end) & (keep != 0) & (sample == 0)) == [k == "use" for k in kinds]
    return keep, sample, start, end


def _likelihoods(rng, n_reads, n_haps):
    m = -np.abs(rng.normal(0.0, 2.0, size=(n_reads, n_haps)))
    m[rng.random(m.shape) < 0.08] = -np.inf
    m[:, 1] = m[:, 0]  # ties between haplotypes
    m[rng.random(m.shape) < 0.05] = 0.0
    return m.reshape(-1)


def _one_event(rng, A, kinds, n_haps, unmapped=None):
    keep, sample, start, end = _reads(rng, kinds)
    b = _Batch([len(kinds)], [n_haps])
    ev = genotype.Events([0], [0, A], [W0], [W1], _hap_map(rng, A, n_haps, unmapped))
    return b, _likelihoods(rng, len(kinds), n_haps), keep, sample, start, end, ev


# ---- the accumulators: G = 256, 257, 512, 513, 768, 769, 1 024 at A = 2 ------------------------------------------------

@pytest.mark.parametrize("ploidy", [255, 256, 511, 512, 767, 768, 1023])
def test_accumulator_boundaries(hip_engine, ploidy):
    rng = np.random.default_rng(ploidy)
    b, L, keep, sample, start, end, ev = _random_case(rng, ploidy, [2, 2, 2], 2, n_reads=40)
    # the third event: allele 1 on no haplotype (its genotypes -inf next to finite ones: PL 2^31 - 1)
    h0, h1 = int(b.region_hap_off[2]), int(b.region_hap_off[3])
    m = ev.hap_allele[h0:h1]
    m[m == 1] = 0
    m[0] = 0
    res = _check(hip_engine, b, L, keep, sample, start, end, ev, ploidy, 2)
    assert res.gl[0].shape == (2, ploidy + 1)
    assert res.gl[2][0, -1] == -np.inf and int(res.n_evidence[2][0]) > 0
    assert np.any(np.isinf(L)) and np.any(np.isfinite(res.gl[0]))


# ---- the tiles: used read counts around T and 2T, with reads dropped by keep, sample and overlap between them -----------

TILE_SHAPES = [(2, 2, 3), (2, 44, 990), (3, 17, 969), (1023, 2, 1024)]


@pytest.mark.parametrize("ploidy,A,G", TILE_SHAPES)
def test_tile_boundaries(hip_engine, ploidy, A, G):
    assert genotype.genotype_count(ploidy, A) == G
    T = _tile(A, G)
    assert T == {3: 256, 990: 3, 969: 4, 1024: 3}[G]
    rng = np.random.default_rng(G)
    n_haps = A + 4
    for n_used in (T - 1, T, T + 1, 2 * T + 1):
        for mixed in (False, True):
            kinds = ["use"] * n_used
            if mixed:  # dropped reads between the used ones, and at both ends
                drops = list(rng.choice(["keep", "sample", "outside"], size=max(3, n_used // 2 + 2)))
                kinds = drops[:1] + kinds + drops[1:2]
                for d in drops[2:]:
                    kinds.insert(int(rng.integers(1, len(kinds))), d)
            res = _check(hip_engine, *_one_event(rng, A, kinds, n_haps), ploidy, 2)
            assert int(res.n_evidence[0][0]) == n_used and int(res.n_evidence[0][1]) == kinds.count("sample")


# ---- many alleles at low ploidy -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("ploidy,A", [(2, 7), (2, 10), (2, 16), (2, 24), (2, 31), (2, 32), (2, 33), (2, 44), (3, 17), (4, 10), (5, 8)])
def test_many_alleles(hip_engine, ploidy, A):
    rng = np.random.default_rng(100 * ploidy + A)
    n_haps = A + 6
    kinds = list(rng.choice(["use", "use", "use", "keep", "sample", "outside"], size=30))
    b, L, keep, sample, start, end, ev = _one_event(rng, A, kinds, n_haps)
    b2, L2, keep2, sample2, start2, end2, ev2 = _one_event(rng, A, kinds, n_haps, unmapped=A - 1)
    b = _Batch([len(kinds)] * 2, [n_haps] * 2)
    ev = genotype.Events([0, 1], [0, A, 2 * A], [W0, W0], [W1, W1], np.concatenate([ev.hap_allele, ev2.hap_allele]))
    cat = np.concatenate
    _check(hip_engine, b, cat([L, L2]), cat([keep, keep2]), cat([sample, sample2]), cat([start, start2]), cat([end, end2]), ev,
           ploidy, 2)
    # and the same shapes through the generic random case (-inf rows, ties, reads of every overlap kind, 3 samples)
    _check(hip_engine, *_random_case(rng, ploidy, [A], 3, n_haps=A + 3), ploidy, 3)


# ---- many samples: the per-sample output offsets ----------------------------------------------------------------------

@pytest.mark.parametrize("n_samples", [64, 200])
def test_many_samples(hip_engine, n_samples):
    rng = np.random.default_rng(n_samples)
    b, L, keep, sample, start, end, ev = _random_case(rng, 2, [2, 3, 5], n_samples, n_reads=2 * n_samples)
    sample[sample % 7 == 3] = 0  # more samples without reads
    res = _check(hip_engine, b, L, keep, sample, start, end, ev, 2, n_samples)
    empty = np.setdiff1d(np.arange(n_samples), sample)
    assert len(empty) >= n_samples // 8
    for e in range(ev.n_events):
        assert np.all(res.n_evidence[e][empty] == 0) and np.all(res.pl[e][empty] == 0) and np.all(res.gl[e][empty] == 0.0)
        assert res.n_evidence[e].sum() > 0


# ---- the limits: ploidy 65 535 and G = 1 024 accepted, ploidy 65 536 and G = 1 025 refused, refusals write nothing -------

def test_limits(hip_engine):
    eng = hip_engine
    rng = np.random.default_rng(7)
    case = _one_event(rng, 1, ["use", "keep", "use", "outside", "use"], 3)
    res = _check(eng, *case, 65535, 2)
    assert res.gl[0].shape == (2, 1) and int(res.n_evidence[0][0]) == 3
    b, L, keep, sample, start, end, ev = case
    ev2 = genotype.Events([0], [0, 2], [W0], [W1], np.array([0, 1, -1], np.int32))

    def run(ploidy, ev):
        gl, pl, ne = np.full(4096, 7.5), np.full(4096, 7, np.int32), np.full(8, 7, np.uint32)
        code = _raw(eng, b, L, keep, sample, start, end, 2, ploidy, ev, np.array([0, 4096], np.uint64), gl, pl, ne)
        return code, gl, pl, ne

    for ploidy, e, ok, why in ((65535, ev, True, None), (65536, ev, False, "ploidy beyond 65535"), (1023, ev2, True, None),
                               (1024, ev2, False, "1025 genotypes, more than 1024")):
        code, gl, pl, ne = run(ploidy, e)
        if ok:
            assert code == _lib.PHMM_OK and gl[0] != 7.5 and ne[0] == 3, ploidy
        else:
            assert code == _lib.PHMM_ERR_INVALID_ARG and why in eng.last_error(), (ploidy, eng.last_error())
            assert np.all(gl == 7.5) and np.all(pl == 7) and np.all(ne == 7), ploidy
