"""phmm_annotate_events on the MI355X: every output equal to the restatement of the reference's annotation step
(tests/annotate_restatement.py) -- integers exact, doubles bit for bit, NaN as NaN -- for seeded batches over sample and
allele counts, call subsets, read counts around the kernel's tile, the edges of the informative threshold, the passes over
samples and call alleles, the BQ inputs present and absent, a shuffled batch against each event alone, the whole
genotyping path end to end, and every refused argument."""
import ctypes as C

import numpy as np
import pytest

import annotate_restatement as A
from lorikeet_amd import _lib, genotype, synthetic
from lorikeet_amd.engine import PhmmError
from test_genotype_edges_hip import W0, W1, _one_event
from test_genotype_hip import _Batch, _random_case, _region_call

pytestmark = pytest.mark.gpu
ANN_MAX_TILE, ANN_LDS_BYTES, ANN_GROUP, ANN_AD_SLOTS, ANN_MAX_CHUNK = 256, 32 * 1024, 8, 2048, 512  # phmm_annotate_internal.hpp
THR = 0.2
_i32p, _i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def _tile(n_call):
    """The kernel's tile: reads one sweep of the workgroup takes."""
    return min(ANN_MAX_TILE, ANN_LDS_BYTES // (8 * n_call))


def _same_f64(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def _subset(rng, A_e, kind):
    """A call's alleles: 'one' (the reference alone), 'two', 'all', 'gapped' (every other allele), 'none' (not annotated)."""
    if kind == "none":
        return []
    if kind == "one" or A_e == 1:
        return [0]
    if kind == "two":
        return [0, int(rng.integers(1, A_e))]
    if kind == "gapped":
        return [0] + list(range(2 if A_e > 2 else 1, A_e, 2))
    return list(range(A_e))


def _aligned(rng, start, end, event_pos):
    """A CIGAR per read that spans [start, end] on the reference out of M = X D N with insertions between them and clips at
    the ends, the qualities of its read bases, the soft start."""
    cigars, quals, soft = [], [], []
    for s, e in zip(start, end):
        left, right = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        text = ("%dH" % rng.integers(1, 5) if rng.random() < 0.2 else "") + ("%dS" % left if left else "")
        remaining, first = int(e) - int(s) + 1, True
        while remaining > 0:
            n = int(rng.integers(1, remaining + 1))
            op = "M" if first else str(rng.choice(list("MMM=XDN")))
            if not first and rng.random() < 0.3:
                text += "%dI" % rng.integers(1, 4)
            text += "%d%s" % (n, op)
            remaining -= n
            first = False
        text += "%dS" % right if right else ""
        cig = A.encode_cigar(text)
        n_bases = sum(int(el) >> 4 for el in cig if A.cigar_consumes_read_bases(int(el) & 15))
        cigars.append(cig)
        quals.append(rng.integers(0, 256 if rng.random() < 0.1 else 61, size=n_bases))
        soft.append(int(s) - left)
    read_off = np.concatenate([[0], np.cumsum([len(q) for q in quals])])
    return genotype.AlignedReads(read_off, np.concatenate(quals) if quals else np.zeros(0), cigars, soft, event_pos)


def _check(eng, b, L, keep, sample, start, end, mapq, ev, calls, err, S, aligned=None, called=None, nf=None, only=None):
    res = genotype.annotate_events(eng, b, L, keep, start, end, sample, mapq, ev, calls, err, n_samples=S, aligned=aligned,
                                   sample_called=called, n_filtered=nf)
    want = A.batch_annotate(b, L, keep, sample, start, end, mapq, S, ev, calls, err, called, nf, aligned, only=only)
    for e, w in want.items():
        tag = (e, ev.n_alleles(e), calls[e])
        assert np.array_equal(res.ad[e], w["ad"]), ("AD", tag, res.ad[e], w["ad"])
        assert np.array_equal(res.dp[e], w["dp"]) and np.array_equal(res.ac[e], w["ac"]), ("DP / AC", tag)
        assert _same_f64(res.af[e], w["af"]), ("AF", tag, res.af[e], w["af"])
        assert np.array_equal(res.mq[e], w["mq"]), ("MQ", tag, res.mq[e], w["mq"])
        if aligned is None:
            assert res.bq is None
        else:
            assert np.array_equal(res.bq[e], w["bq"]), ("BQ", tag, res.bq[e], w["bq"])
        assert int(res.info_dp[e]) == w["info_dp"] and int(res.qd_depth[e]) == w["qd_depth"], ("depth", tag, res.qd_depth[e], w["qd_depth"])
        assert _same_f64(res.qd[e:e + 1], [w["qd"]]) and int(res.flags[e]) == w["flags"], ("QD", tag, res.qd[e], w["qd"], res.flags[e], w["flags"])
    return res


def _extras(rng, n_reads, n_events, S):
    """mapq with zeros, log10_p_error with NaN and the reference's 1.0, no-calls, filtered-read counts."""
    mapq = rng.integers(1, 61, size=n_reads).astype(np.uint8)
    mapq[rng.random(n_reads) < 0.15] = 0
    err = -rng.random(n_events) * 40.0
    err[rng.random(n_events) < 0.1] = np.nan
    err[rng.random(n_events) < 0.05] = 1.0
    called = (rng.random((n_events, S)) > 0.2).astype(np.uint8)
    nf = rng.integers(0, 5, size=(n_events, S)).astype(np.uint32)
    return mapq, err, called, nf


@pytest.mark.parametrize("n_samples", [1, 3, 200])
def test_random_batches_equal(hip_engine, n_samples):
    kinds = ["one", "two", "all", "gapped", "none"]
    for seed in (1, 2):
        rng = np.random.default_rng(seed * 100 + n_samples)
        alleles = [2, 3, 4, 5, 8, 9, 16, 17, 33, 44, 2, 3, 7, 12, 44]
        b, L, keep, sample, start, end, ev = _random_case(rng, 2, alleles, n_samples, n_reads=24 if n_samples < 200 else 420)
        calls = [_subset(rng, ev.n_alleles(e), kinds[(e + seed) % 5]) for e in range(ev.n_events)]
        mapq, err, called, nf = _extras(rng, b.n_reads, ev.n_events, n_samples)
        pos = (ev.start + 2 + rng.integers(-1, 2, size=ev.n_events)).astype(np.int64)
        al = _aligned(rng, start, end, pos)
        res = _check(hip_engine, b, L, keep, sample, start, end, mapq, ev, calls, err, n_samples, al, called, nf)
        assert any(np.isnan(a).any() for a in res.af) or n_samples == 1  # a sample without reads: 0 / 0
        assert sum(int(a.sum()) for a in res.ad) > 0 and any((m != 30).any() for m in res.mq) and any((q != 30).any() for q in res.bq)
        # ... and the optional inputs absent: no BQ, every sample called, no filtered reads
        _check(hip_engine, b, L, None, sample, start, end, mapq, ev, calls, err, n_samples)


@pytest.mark.parametrize("A_e", [2, 9, 17, 44])
def test_tile_boundaries(hip_engine, A_e):
    T = _tile(A_e)
    assert T == {2: 256, 9: 256, 17: 240, 44: 93}[A_e]
    rng = np.random.default_rng(A_e)
    for n_used in (T - 1, T, T + 1, 2 * T + 1):
        for mixed in (False, True):
            kinds = ["use"] * n_used
            if mixed:  # dropped reads between the used ones, and at both ends
                drops = list(rng.choice(["keep", "sample", "outside"], size=max(3, n_used // 2 + 2)))
                kinds = drops[:1] + kinds + drops[1:2]
                for d in drops[2:]:
                    kinds.insert(int(rng.integers(1, len(kinds))), d)
            b, L, keep, sample, start, end, ev = _one_event(rng, A_e, kinds, A_e + 4)
            mapq, err, _, _ = _extras(rng, len(kinds), 1, 2)
            al = _aligned(rng, start, end, [W0 + 2])
            res = _check(hip_engine, b, L, keep, sample, start, end, mapq, ev, [list(range(A_e))], [-20.0], 2, al)
            assert int(res.dp[0][0]) <= n_used and int(res.dp[0][1]) <= kinds.count("sample")


def test_tiles_of_unequal_calls_in_one_batch(hip_engine):
    """The launch sizes the LDS tile once per batch: calls of 16 alleles (T = 256, 4 096 doubles) beside 17 (T = 240, 4 080)
    and 2, each with more used reads than its tile."""
    rng = np.random.default_rng(1617)
    parts = [_one_event(rng, A_e, ["use"] * 300, A_e + 2) for A_e in (17, 16, 2, 16)]
    b = _Batch([300] * 4, [p[6].hap_allele.size for p in parts])
    cat = lambda i: np.concatenate([p[i] for p in parts])  # noqa: E731
    n_al = [17, 16, 2, 16]
    ev = genotype.Events([0, 1, 2, 3], np.concatenate([[0], np.cumsum(n_al)]), [W0] * 4, [W1] * 4, np.concatenate([p[6].hap_allele for p in parts]))
    mapq, err, called, nf = _extras(rng, 1200, 4, 1)
    _check(hip_engine, b, cat(1), cat(2), cat(3), cat(4), cat(5), mapq, ev, [list(range(a)) for a in n_al], err, 1,
           _aligned(rng, cat(4), cat(5), [W0 + 2] * 4), called, nf)


def _planted(rng, n_alleles, n_reads):
    """One haplotype per allele; per read one of: as drawn, an exact tie with the best, another allele at exactly best - 0.2 or
    one ulp either side of it, the reference that far from the best, -inf entries, a row of -inf, values on a grid of 0.2."""
    v = -np.abs(rng.normal(0.0, 1.0, size=(n_reads, n_alleles)))
    for r in range(n_reads):
        kind = r % 9
        bst = int(np.argmax(v[r]))
        other = int(rng.integers(0, n_alleles))
        if kind in (1, 2, 3, 4) and other != bst:
            v[r, other] = v[r, bst] - [0.0, THR, np.nextafter(THR, 0.0), np.nextafter(THR, 1.0)][kind - 1]
        elif kind == 5 and bst != 0:
            v[r, 0] = v[r, bst] - [THR, np.nextafter(THR, 0.0), np.nextafter(THR, 1.0), 0.0][r // 9 % 4]
        elif kind == 6:
            v[r, rng.random(n_alleles) < 0.5] = -np.inf
        elif kind == 7:
            v[r, :] = -np.inf
        elif kind == 8:
            v[r] = np.round(v[r] * 5) / 5
    return v


@pytest.mark.parametrize("A_e", [2, 3, 6, 20])
def test_ties_and_the_threshold_to_the_ulp(hip_engine, A_e):
    rng = np.random.default_rng(40 + A_e)
    n = 540
    v = _planted(rng, A_e, n)
    b = _Batch([n] * 4, [A_e] * 4)
    ident = np.arange(A_e, dtype=np.int32)
    no_last = ident.copy()
    no_last[-1] = -1  # an allele no haplotype maps to: its row is -inf for every read
    ev = genotype.Events([0, 1, 2, 3], np.arange(5) * A_e, [W0] * 4, [W1] * 4, np.concatenate([ident, ident, no_last, ident]))
    calls = [list(range(A_e)), _subset(rng, A_e, "two"), list(range(A_e)), [0]]
    start, end = np.full(4 * n, W0 - 3, np.int64), np.full(4 * n, W1 + 3, np.int64)
    mapq = np.tile(rng.integers(0, 4, size=n).astype(np.uint8) * 20, 4)
    sample = np.tile((np.arange(n) % 2).astype(np.uint32), 4)
    res = _check(hip_engine, b, np.tile(v.reshape(-1), 4), None, sample, start, end, mapq, ev, calls, [-30.0, -8.0, np.nan, -1.0], 2)
    assert int(res.flags[3]) & _lib.PHMM_ANN_NO_AD and int(res.flags[2]) & _lib.PHMM_ANN_NO_QD
    assert 0 < int(res.info_dp[0]) < n  # some reads informative, some not


@pytest.mark.parametrize("S,A_e", [(200, 44), (600, 2), (513, 5), (47, 44)])
def test_passes_over_samples_and_call_alleles(hip_engine, S, A_e):
    """2 048 / C samples (at most 512) and 8 call alleles per pass: several chunks of samples, several groups of alleles."""
    chunk = min(ANN_MAX_CHUNK, ANN_AD_SLOTS // A_e)
    assert -(-S // chunk) >= 2 or -(-A_e // ANN_GROUP) >= 2
    rng = np.random.default_rng(S + A_e)
    n, nh = 3 * S + 50 + 40 * A_e, A_e + 3
    b = _Batch([n], [nh])
    L = -np.abs(rng.normal(0.0, 1.5, size=n * nh))
    sample = rng.integers(0, S, size=n).astype(np.uint32)
    start = rng.integers(0, 50, size=n).astype(np.int64)
    ev = genotype.Events([0], [0, A_e], [W0], [W1], np.concatenate([rng.permutation(A_e), rng.integers(-1, A_e, size=3)]))
    mapq, err, called, nf = _extras(rng, n, 1, S)
    al = _aligned(rng, start, start + 30, [W0 + 1])
    res = _check(hip_engine, b, L, None, sample, start, start + 30, mapq, ev, [list(range(A_e))], [-50.0], S, al, called, nf)
    assert int(res.info_dp[0]) == int(res.dp[0].sum()) > 0


def test_events_without_used_reads(hip_engine):
    rng = np.random.default_rng(8)
    b = _Batch([12], [4])
    L = -np.abs(rng.normal(size=48))
    start = np.full(12, 500, np.int64)
    ev = genotype.Events([0, 0], [0, 3, 6], [W0, W0], [W1, W1], [0, 1, 2, 1, 0, 1, 2, 1])
    nf = np.array([[0, 0], [4, 1]], np.uint32)
    res = _check(hip_engine, b, L, None, np.zeros(12, np.uint32), start, start + 20, np.full(12, 60, np.uint8), ev, [[0, 1, 2], [0, 2]],
                 [-9.0, -9.0], 2, nf=nf)
    assert not res.ad[0].any() and np.isnan(res.af[0]).all() and list(res.mq[0]) == [30, 30, 30]
    assert int(res.flags[0]) == _lib.PHMM_ANN_NO_QD and res.qd[0] == 0.0 and int(res.qd_depth[0]) == 0
    assert int(res.qd_depth[1]) == 5 and res.qd[1] == 90.0 / 5.0 and int(res.flags[1]) == 0  # the filtered reads stand in


def test_qd_jitter_on_both_sides_of_45(hip_engine):
    # three reads, all informative for the alternate allele: depth 3; QD = -10 e / 3
    L = np.array([[-9.0, -1.0]] * 3).reshape(-1)
    b = _Batch([3] * 3, [2] * 3)
    ev = genotype.Events([0, 1, 2], [0, 2, 4, 6], [W0] * 3, [W1] * 3, [0, 1] * 3)
    err = np.array([-13.5, np.nextafter(-13.5, 0.0), np.nextafter(-13.5, -20.0)])
    start = np.full(9, W0, np.int64)
    res = _check(hip_engine, b, np.tile(L, 3), None, np.zeros(9, np.uint32), start, start + 5, np.full(9, 60, np.uint8), ev, [[0, 1]] * 3, err, 1)
    assert list(res.qd_depth) == [3, 3, 3] and res.qd[0] == 45.0 and res.qd[1] < 45.0 < res.qd[2]
    assert [int(f) for f in res.flags] == [_lib.PHMM_ANN_QD_JITTER, 0, _lib.PHMM_ANN_QD_JITTER]


def test_shuffled_mixed_batch_equals_each_event_alone(hip_engine):
    rng = np.random.default_rng(21)
    G = 60
    nr, nh = rng.integers(4, 300, size=G), rng.integers(2, 12, size=G)
    b = _Batch(nr, nh)
    n = b.n_reads
    L = -np.abs(rng.normal(0, 2, size=int(b.out_off[-1])))
    L[rng.random(L.shape) < 0.03] = -np.inf
    sample, keep = rng.integers(0, 3, size=n).astype(np.uint32), (rng.random(n) > 0.05).astype(np.uint8)
    start = rng.integers(0, 100, size=n).astype(np.int64)
    end = start + rng.integers(0, 60, size=n)
    region, a_off, w, maps, calls = [], [0], [], [], []
    for g in rng.permutation(np.repeat(np.arange(G), 4)):  # four events per region, in a shuffled order
        A_e = int(rng.choice([2, 3, 5, 9, 20]))
        region.append(int(g))
        a_off.append(a_off[-1] + A_e)
        w.append(int(rng.integers(0, 150)))
        maps.append(rng.integers(-1, A_e, size=int(nh[g])))
        calls.append(_subset(rng, A_e, str(rng.choice(["one", "two", "all", "gapped", "none"]))))
    ev = genotype.Events(region, a_off, np.array(w) - 2, np.array(w) + 2, np.concatenate(maps))
    mapq, err, called, nf = _extras(rng, n, ev.n_events, 3)
    al = _aligned(rng, start, end, np.array(w))
    whole = _check(hip_engine, b, L, keep, sample, start, end, mapq, ev, calls, err, 3, al, called, nf, only=list(range(0, ev.n_events, 7)))
    moff = np.concatenate([[0], np.cumsum(nh[np.asarray(region)])])
    for e in range(ev.n_events):
        g = region[e]
        r0, r1 = int(b.region_read_off[g]), int(b.region_read_off[g + 1])
        lo = int(b.out_off[g])
        e1 = genotype.Events([0], [0, ev.n_alleles(e)], ev.start[e:e + 1], ev.end[e:e + 1], ev.hap_allele[moff[e]:moff[e + 1]])
        cig = [al.cigar[int(al.cigar_off[r]):int(al.cigar_off[r + 1])] for r in range(r0, r1)]
        a1 = genotype.AlignedReads(al.read_off[r0:r1 + 1] - al.read_off[r0], al.base_q[int(al.read_off[r0]):int(al.read_off[r1])], cig,
                                   al.soft_start[r0:r1], al.event_pos[e:e + 1])
        part = genotype.annotate_events(hip_engine, _Batch([nr[g]], [nh[g]]), L[lo:lo + int(nr[g] * nh[g])], keep[r0:r1], start[r0:r1],
                                        end[r0:r1], sample[r0:r1], mapq[r0:r1], e1, [calls[e]], err[e:e + 1], n_samples=3, aligned=a1,
                                        sample_called=called[e:e + 1], n_filtered=nf[e:e + 1])
        assert np.array_equal(part.ad[0], whole.ad[e]) and _same_f64(part.af[0], whole.af[e]) and np.array_equal(part.dp[0], whole.dp[e])
        assert np.array_equal(part.ac[0], whole.ac[e]) and np.array_equal(part.mq[0], whole.mq[e]) and np.array_equal(part.bq[0], whole.bq[e])
        assert (int(part.info_dp[0]), int(part.qd_depth[0]), int(part.flags[0])) == (int(whole.info_dp[e]), int(whole.qd_depth[e]), int(whole.flags[e]))
        assert _same_f64(part.qd, whole.qd[e:e + 1])


def test_end_to_end_from_the_region_call(hip_engine):
    """phmm_region_compute -> phmm_genotype_likelihoods -> phmm_allele_frequency -> phmm_annotate_events, the call's alleles taken
    from the OUTPUT flags and log10_p_error from QUAL, against the restatement fed the same way."""
    batch = synthetic.make_regions(6, 40, 4, 120, [50, 70], seed=77)
    one, ref_start = _region_call(hip_engine, batch, 77)
    orig_start = np.repeat(ref_start, np.diff(batch.region_read_off.astype(np.int64)))
    moved = one.reads.status == 0
    start = np.where(moved, one.reads.new_pos, orig_start).astype(np.int64)
    cigars = [c if m else A.encode_cigar("%dM" % (batch.read_off[r + 1] - batch.read_off[r])) for r, (c, m) in enumerate(zip(one.reads.cigars, moved))]
    end = np.array([genotype.read_end(p, c) for p, c in zip(start, cigars)], np.int64)
    soft = np.array([int(p) - (int(c[0]) >> 4 if len(c) and int(c[0]) & 15 == 4 else 0) for p, c in zip(start, cigars)], np.int64)
    ev = synthetic.make_events(batch, region_reference_start=ref_start)
    sample = (np.arange(batch.n_reads) % 2).astype(np.uint32)
    keep = one.keep.astype(np.uint8)
    gt = genotype.genotype_likelihoods(hip_engine, batch, one.likelihoods, keep, start, end, sample, ev, ploidy=2, n_samples=2)
    af = genotype.allele_frequency(hip_engine, gt, allele_off=ev.allele_off, allele_length=np.ones(int(ev.allele_off[-1]), np.uint32))
    calls = genotype.call_alleles_of(af)
    assert sum(1 for c in calls if len(c) >= 2) >= 1
    err = af.qual / -10.0
    al = genotype.AlignedReads(batch.read_off, batch.base_q, cigars, soft, ev.start + 2)
    mapq = np.full(batch.n_reads, 60, np.uint8)
    mapq[::7] = 0
    res = _check(hip_engine, batch, one.likelihoods, keep, sample, start, end, mapq, ev, calls, err, 2, al)
    assert int(res.info_dp.sum()) > 0 and any(len(q) and (q != 30).any() for q in res.bq)


_NAMES = ["region_read_off", "region_hap_off", "out_off", "likelihoods", "keep", "read_sample", "read_start", "read_end", "mapq",
          "event_region", "event_allele_off", "event_start", "event_end", "event_hap_allele", "call_allele_off", "call_allele",
          "read_off", "base_q", "out_cigar_off", "out_cigar", "n_out_cigar", "read_soft_start", "event_pos", "sample_called",
          "log10_p_error", "n_filtered", "ad", "dp", "af", "ac", "mq", "bq", "info_dp", "qd_depth", "qd", "flags"]
_OUTPUTS = _NAMES[26:]
_TYPES = dict(out_off=np.uint64, likelihoods=np.float64, keep=np.uint8, read_start=np.int64, read_end=np.int64, mapq=np.uint8,
              event_start=np.int64, event_end=np.int64, event_hap_allele=np.int32, base_q=np.uint8, out_cigar_off=np.uint64,
              read_soft_start=np.int64, event_pos=np.int64, sample_called=np.uint8, log10_p_error=np.float64, ad=np.int32,
              dp=np.int32, af=np.float64, mq=np.uint8, bq=np.uint8, info_dp=np.int32, qd_depth=np.int32, qd=np.float64)
_CT = {np.uint8: _lib.u8p, np.uint32: _lib.u32p, np.uint64: _lib.u64p, np.int32: _i32p, np.int64: _i64p, np.float64: _lib.f64p}


def _raw(eng, n_regions, n_samples, n_events, arrays):
    """phmm_annotate_events on a dict of arrays by parameter name (None: NULL)."""
    a = {k: None if arrays.get(k) is None else np.ascontiguousarray(arrays[k], _TYPES.get(k, np.uint32)) for k in _NAMES}
    for k in _OUTPUTS:  # the caller's own buffers, so that it can look at them afterwards
        a[k] = arrays.get(k)
    p = [None if a[k] is None else a[k].ctypes.data_as(_CT[_TYPES.get(k, np.uint32)]) for k in _NAMES]
    return eng.lib.phmm_annotate_events(eng._h, n_regions, *p[:9], n_samples, n_events, *p[9:])


def test_invalid_arguments_write_nothing(hip_engine):
    eng = hip_engine
    L = np.array([-9.0, -1.0] * 4 + [-9.0, -5.0, -1.0] * 3)  # every read informative for its region's last allele

    def good():
        return dict(region_read_off=[0, 4, 7], region_hap_off=[0, 2, 5], out_off=[0, 8, 17], likelihoods=L, keep=None,
                    read_sample=np.zeros(7), read_start=np.zeros(7), read_end=np.full(7, 10), mapq=np.full(7, 60),
                    event_region=[0, 1], event_allele_off=[0, 2, 5], event_start=[0, 0], event_end=[5, 5],
                    event_hap_allele=[0, 1, 0, 1, 2], call_allele_off=[0, 2, 4], call_allele=[0, 1, 0, 2],
                    read_off=np.arange(8) * 11, base_q=np.full(77, 41), out_cigar_off=np.arange(8) * 2, out_cigar=np.tile([11 << 4, 0], 7),
                    n_out_cigar=np.ones(7), read_soft_start=np.zeros(7), event_pos=[2, 3], sample_called=None, log10_p_error=[-5.0, -6.0],
                    n_filtered=None)

    def run(n_regions=2, n_samples=1, n_events=2, **change):
        arrays = good()
        arrays.update(change)
        outs = dict(ad=np.full(8, 7, np.int32), dp=np.full(4, 7, np.int32), af=np.full(8, 7.5), ac=np.full(4, 7, np.uint32),
                    mq=np.full(8, 7, np.uint8), bq=np.full(8, 7, np.uint8), info_dp=np.full(4, 7, np.int32),
                    qd_depth=np.full(4, 7, np.int32), qd=np.full(4, 7.5), flags=np.full(4, 7, np.uint32))
        for k in _OUTPUTS:
            arrays[k] = None if (k in change and change[k] is None) else outs[k]
        code = _raw(eng, n_regions, n_samples, n_events, arrays)
        return code, all(np.all(v == (7.5 if v.dtype == np.float64 else 7)) for v in outs.values()), outs

    code, untouched, outs = run()
    assert code == _lib.PHMM_OK and not untouched, eng.last_error()
    assert list(outs["ad"][:4]) == [0, 4, 0, 3] and list(outs["bq"][:4]) == [30, 41, 30, 41] and list(outs["dp"][:2]) == [4, 3]
    code, untouched, outs = run(**{k: None for k in ("read_off", "base_q", "out_cigar_off", "out_cigar", "n_out_cigar", "read_soft_start",
                                                     "event_pos", "bq")})
    assert code == _lib.PHMM_OK and list(outs["mq"][:4]) == [30, 60, 30, 60]  # the BQ arrays NULL together: no BQ
    bad = {
        "call_allele[0] is not 0": dict(call_allele=[0, 1, 1, 2]),
        "outside [0, A_e)": dict(call_allele=[0, 1, 0, 3]),
        "not strictly increasing": dict(call_allele_off=[0, 1, 4], call_allele=[0, 0, 2, 2]),
        "call_allele_off not monotonic": dict(call_allele_off=[0, 2, 1]),
        "event_allele_off not monotonic": dict(event_allele_off=[0, 2, 1]),
        "no alleles": dict(event_allele_off=[0, 2, 2], call_allele_off=[0, 2, 2]),
        "more than 1024": dict(event_allele_off=[0, 2, 1027]),
        "maps outside": dict(event_hap_allele=[0, 1, 0, 3, 2]),
        "event 1: haplotype 0 maps outside": dict(event_hap_allele=[0, 1, -2, 1, 2]),
        "event_region outside": dict(event_region=[0, 2]),
        "read_sample outside": dict(read_sample=[0, 0, 0, 1, 0, 0, 0]),
        "region offsets not monotonic": dict(region_read_off=[0, 4, 3]),
        "must start at 0": dict(region_hap_off=[1, 2, 5]),
        "n_out_cigar beyond": dict(n_out_cigar=[1, 1, 3, 1, 1, 1, 1]),
        "read_off not monotonic": dict(read_off=[0, 11, 5, 33, 44, 55, 66, 77]),
    }
    for name in ("read_off", "base_q", "out_cigar_off", "out_cigar", "n_out_cigar", "read_soft_start", "event_pos", "bq"):
        bad["BQ arrays|" + name] = {name: None}  # given in part
    for name in ("region_read_off", "region_hap_off", "out_off", "likelihoods", "read_sample", "read_start", "read_end", "mapq",
                 "event_region", "event_allele_off", "event_start", "event_end", "event_hap_allele", "call_allele_off", "call_allele",
                 "log10_p_error", "ad", "dp", "af", "ac", "mq", "info_dp", "qd_depth", "qd", "flags"):
        bad["null array|" + name] = {name: None}
    for what, change in bad.items():
        code, untouched, _ = run(**change)
        assert code == _lib.PHMM_ERR_INVALID_ARG and untouched, what
        assert eng.last_error().startswith("phmm_annotate_events") and what.split("|")[0] in eng.last_error(), (what, eng.last_error())
    code, untouched, _ = run(n_events=0)
    assert code == _lib.PHMM_OK and untouched
    assert "event 1" in (run(call_allele=[0, 1, 0, 3]), eng.last_error())[1]
    b = _Batch([4], [2])
    with pytest.raises(PhmmError):
        genotype.annotate_events(eng, b, L[:8], None, np.zeros(4), np.ones(4), np.zeros(4), np.full(4, 60), genotype.Events([0], [0, 2], [0], [5], [0, 1]),
                                 [[1]], [-3.0])
