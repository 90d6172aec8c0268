"""The grow path of the staging buffers (StagingBuffer::grow, lorikeet_amd/csrc/phmm_staging.hpp) under the five entry points
that lay their arrays out with a StageLayout: phmm_project_to_reference, phmm_genotype_likelihoods, phmm_allele_frequency,
phmm_annotate_events, phmm_assign_genotypes.

A buffer starts at 1 MiB and the session's engine has long outgrown whatever the other modules need, so each case here makes
its own engine and calls the entry point three times: a small case its own module checks against the restatement or the
oracle (the buffer's first allocation), the same case K times over in one call (K the smallest count at which one input array
alone passes 1 MiB: the buffer has to grow), and the small case again (the grown buffer, reused).  Every copy inside the large
call and the third call must give the first call's outputs bit for bit -- the kernels compute an event, or a read, the same
way whatever else is in the batch (the modules' batch-invariance tests) -- and the first and the third call must stage the
same number of input bytes.  No tolerance anywhere."""
import numpy as np
import pytest

from lorikeet_amd import HipPairHMMEngine, genotype, realign
from lorikeet_amd.batch import RegionBatch
from project_scenarios import scenario
from test_af_hip import R as AF, _grid_events, _run as af_run
from test_annotate_hip import _aligned, _extras, _subset
from test_assign_hip import POSTERIOR_SEED, R as AS, posterior_events, run as assign_run, same_f64
from test_genotype_hip import _Batch, _random_case

pytestmark = pytest.mark.gpu
FLOOR = 1 << 20  # bytes a staging buffer has after its first allocation at least


def copies_to_outgrow(array):
    """The smallest K at which K copies of `array` are more than FLOOR bytes."""
    return FLOOR // np.asarray(array).nbytes + 1


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if want.dtype == np.float64:
        return got.dtype == np.float64 and same_f64(got, want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def tile_off(off, K):
    """An offset array [n + 1] for K copies of its n items."""
    return np.concatenate([[0], np.cumsum(np.tile(np.diff(np.asarray(off).astype(np.int64)), K))])


def grow_and_compare(small, large, fields, n_items, K):
    """small(eng) / large(eng): the calls; fields(result): [(name, per-item sequence)]; n_items: items (events, reads) of the
    small case, item i of copy k being item k * n_items + i of the large call."""
    eng = HipPairHMMEngine(0)
    try:
        s0 = eng.stat("staged_bytes")
        first = fields(small(eng))
        s1 = eng.stat("staged_bytes")
        many = fields(large(eng))
        s2 = eng.stat("staged_bytes")
        third = fields(small(eng))
        s3 = eng.stat("staged_bytes")
    finally:
        eng.close()
    assert [n for n, _ in first] == [n for n, _ in many] == [n for n, _ in third]
    for (name, one), (_, all_), (_, again) in zip(first, many, third):
        assert len(one) == n_items and len(all_) == K * n_items and len(again) == n_items, (name, len(one), len(all_))
        for i in range(n_items):
            assert same(again[i], one[i]), (name, "third call", i)
        for j in range(K * n_items):
            assert same(all_[j], one[j % n_items]), (name, "copy", j // n_items, "item", j % n_items)
    assert s3 - s2 == s1 - s0, ("staged bytes of the first and the third call", s1 - s0, s3 - s2)
    return s1 - s0, s2 - s1


def _region_case(seed, n_samples):
    b, L, keep, sample, start, end, ev = _random_case(np.random.default_rng(seed), 2, [2, 3, 5], n_samples)
    K = copies_to_outgrow(L)
    reads, haps = np.diff(b.region_read_off.astype(np.int64)), np.diff(b.region_hap_off.astype(np.int64))
    bK = _Batch(np.tile(reads, K), np.tile(haps, K))
    region = np.concatenate([ev.region.astype(np.int64) + k * b.n_regions for k in range(K)])
    evK = genotype.Events(region, tile_off(ev.allele_off, K), np.tile(ev.start, K), np.tile(ev.end, K), np.tile(ev.hap_allele, K))
    one = (b, L, keep, start, end, sample)
    many = (bK, np.tile(L, K), np.tile(keep, K), np.tile(start, K), np.tile(end, K), np.tile(sample, K))
    return K, one, ev, many, evK


def test_genotype_likelihoods():
    S = 3
    K, one, ev, many, evK = _region_case(31, S)
    staged, staged_large = grow_and_compare(
        lambda eng: genotype.genotype_likelihoods(eng, *one, ev, ploidy=2, n_samples=S),
        lambda eng: genotype.genotype_likelihoods(eng, *many, evK, ploidy=2, n_samples=S),
        lambda r: [("gl", r.gl), ("pl", r.pl), ("n_evidence", r.n_evidence)], ev.n_events, K)
    assert staged > 0 and staged_large > FLOOR


def test_annotate_events():
    S = 3
    K, one, ev, many, evK = _region_case(32, S)
    b, _, _, start, end, _ = one
    rng = np.random.default_rng(33)
    calls = [_subset(rng, ev.n_alleles(e), kind) for e, kind in enumerate(["all", "two", "gapped"])]
    mapq, err, called, nf = _extras(rng, b.n_reads, ev.n_events, S)
    al = _aligned(rng, start, end, (ev.start + 2).astype(np.int64))
    cigars = [al.cigar[int(al.cigar_off[r]):int(al.cigar_off[r + 1])] for r in range(b.n_reads)]
    alK = genotype.AlignedReads(tile_off(al.read_off, K), np.tile(al.base_q, K), cigars * K, np.tile(al.soft_start, K), np.tile(al.event_pos, K))
    fields = lambda r: [("ad", r.ad), ("af", r.af), ("dp", r.dp), ("ac", r.ac), ("mq", r.mq), ("bq", r.bq), ("info_dp", r.info_dp),  # noqa: E731
                        ("qd_depth", r.qd_depth), ("qd", r.qd), ("flags", r.flags)]
    staged, staged_large = grow_and_compare(
        lambda eng: genotype.annotate_events(eng, *one, mapq, ev, calls, err, n_samples=S, aligned=al, sample_called=called, n_filtered=nf),
        lambda eng: genotype.annotate_events(eng, *many, np.tile(mapq, K), evK, calls * K, np.tile(err, K), n_samples=S, aligned=alK,
                                             sample_called=np.tile(called, (K, 1)), n_filtered=np.tile(nf, (K, 1))),
        fields, ev.n_events, K)
    assert staged > 0 and staged_large > FLOOR


def test_allele_frequency():
    S, ploidy, rng = 16, 2, np.random.default_rng(34)
    events = [e for A in range(2, 7) for e in _grid_events(rng, ploidy, A, S)]
    K = copies_to_outgrow(np.concatenate([np.asarray(e[2], np.int32).reshape(-1) for e in events]))
    fields = lambda r: [("log10_p_no_variant", r.log10_p_no_variant), ("log10_p_variant_present", r.log10_p_variant_present),  # noqa: E731
                        ("qual", r.qual), ("flags", r.flags), ("iterations", r.iterations), ("log10_p_absent", r.log10_p_absent),
                        ("mle_count", r.mle_count), ("allele_flags", r.allele_flags)]
    staged, staged_large = grow_and_compare(lambda eng: af_run(eng, events, S, ploidy, AF.pseudo_counts()),
                                            lambda eng: af_run(eng, events * K, S, ploidy, AF.pseudo_counts()), fields, len(events), K)
    assert staged > 0 and staged_large > FLOOR


def test_assign_genotypes():
    ploidy, S, events = next(c for c in posterior_events(POSTERIOR_SEED) if c[0] == 2 and c[1] == 3)
    K = copies_to_outgrow(np.concatenate([np.asarray(e.pls, np.int32).reshape(-1) for e in events]))
    fields = lambda r: [("sub_pl", r.sub_pl), ("gt", r.gt), ("gq", r.gq), ("log10_gq", r.log10_gq), ("sample_called", r.sample_called),  # noqa: E731
                        ("sample_flags", r.sample_flags), ("gp", r.gp), ("pg", r.pg), ("log10_p_error_posterior", r.log10_p_error_posterior)]
    staged, staged_large = grow_and_compare(lambda eng: assign_run(eng, events, S, ploidy, AS.USE_POSTERIORS),
                                            lambda eng: assign_run(eng, events * K, S, ploidy, AS.USE_POSTERIORS), fields, len(events), K)
    assert staged > 0 and staged_large > FLOOR


def test_project_to_reference(hip_engine):
    """(The session's engine makes the inputs -- likelihoods, best alleles, alignments; the projection runs on an engine of
    its own.  A read the projection refuses has its status and nothing else: position and CIGAR are compared for the others.)"""
    b, hap_cigars, hap_starts, ref_hap, ref_start, orig_cigars = scenario(1)
    best, aligned = realign.realign_reads_to_their_best_haplotype(hip_engine, b, hip_engine.compute(b))
    K = copies_to_outgrow(b.read_bases)
    bK = RegionBatch.concat([b] * K)

    def fields(r):
        ok = r.status == 0
        assert ok.any()
        return [("status", r.status), ("new_pos", np.where(ok, r.new_pos, 0)),
                ("cigar", [c if good else c[:0] for c, good in zip(r.cigars, ok)])]
    grow_and_compare(
        lambda eng: realign.project_to_reference(eng, b, best.allele_index, aligned, hap_cigars, hap_starts, ref_hap, ref_start, orig_cigars,
                                                 capacity=64),
        lambda eng: realign.project_to_reference(eng, bK, np.tile(best.allele_index, K), aligned * K, hap_cigars * K, hap_starts * K,
                                                 ref_hap * K, ref_start * K, orig_cigars * K, capacity=64),
        fields, b.n_reads, K)
