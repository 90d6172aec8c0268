"""Per-event genotype likelihoods over the C ABI (phmm_genotype_likelihoods, include/phmm.h): the last arithmetic step of the
reference's call_region, genotyping_engine.assign_genotype_likelihoods (src/haplotype/haplotype_caller_engine.rs:1379) --
marginalization of the likelihood matrix to each event's alleles, the reads of each sample that overlap the event window,
and GenotypeLikelihoodCalculator::genotype_likelihoods (src/genotype/genotype_likelihood_calculator.rs:308-580) with the
PLs of Genotype::build_from_likelihoods.  Everything runs on the MI355X; this file only moves pointers."""
import ctypes as C
import itertools

import numpy as np

from . import _lib
from .engine import PhmmError

ALLELE_INFORMATIVE_READS_OVERLAP_MARGIN = 2  # --allele-informative-reads-overlap-margin (haplotype_caller_genotyping_engine.rs:217-229)
MAX_GENOTYPE_COUNT = 1024  # max_genotype_count_to_enumerate (haplotype_caller_genotyping_engine.rs:66)
_REFERENCE_OPS = (0, 2, 3, 7, 8)  # M, D, N, =, X: what CigarUtils::get_reference_length counts (src/reads/cigar_utils.rs:608-623)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def genotype_count(ploidy, n_alleles):
    """Genotypes of `ploidy` over `n_alleles` alleles (phmm_genotype_count: saturates at 2^32 - 1)."""
    return int(_lib.load().phmm_genotype_count(int(ploidy), int(n_alleles)))


def genotype_allele_counts(ploidy, n_alleles):
    """Every genotype in the reference's index order, as its distinct alleles ascending with their counts:
    [((allele, count), ...), ...] -- diploid over 3 alleles: 0/0, 0/1, 1/1, 0/2, 1/2, 2/2.  The index of the sorted alleles
    a_1 <= ... <= a_p is sum offset[i][a_i] (build_allele_first_genotype_offset_table, allele_heap_to_index)."""
    g = genotype_count(ploidy, n_alleles)
    if g > MAX_GENOTYPE_COUNT:
        raise ValueError("%d genotypes: more than %d" % (g, MAX_GENOTYPE_COUNT))
    off = np.zeros((ploidy + 1, n_alleles + 1), np.int64)
    off[0, 1:] = 1
    for p in range(1, ploidy + 1):
        for a in range(1, n_alleles + 1):
            off[p, a] = off[p, a - 1] + off[p - 1, a]
    out = [None] * g
    for alleles in itertools.combinations_with_replacement(range(n_alleles), ploidy):
        counts = np.bincount(np.asarray(alleles, np.int64), minlength=n_alleles)
        out[sum(int(off[i + 1, x]) for i, x in enumerate(alleles))] = tuple((b, int(c)) for b, c in enumerate(counts) if c)
    return out


def read_end(new_pos, cigar):
    """BirdToolRead::get_end (src/reads/bird_tool_reads.rs:239-249): start + max(reference length - 1, 0) for BAM-encoded
    CIGAR elements ((length << 4) | op)."""
    c = np.asarray(cigar, np.uint32)
    ref_len = int(sum(int(e >> 4) for e in c if int(e & 15) in _REFERENCE_OPS))
    return int(new_pos) + max(ref_len - 1, 0)


class Events:
    """The variant events of a batch: region, alleles (allele_off prefix sums), closed window, haplotype -> allele map
    (one entry per haplotype of the event's region, concatenated in event order; -1 = none)."""

    def __init__(self, region, allele_off, start, end, hap_allele):
        self.region = np.ascontiguousarray(region, np.uint32)
        self.allele_off = np.ascontiguousarray(allele_off, np.uint32)
        self.start = np.ascontiguousarray(start, np.int64)
        self.end = np.ascontiguousarray(end, np.int64)
        self.hap_allele = np.ascontiguousarray(hap_allele, np.int32)

    @property
    def n_events(self):
        return len(self.region)

    def n_alleles(self, e):
        return int(self.allele_off[e + 1]) - int(self.allele_off[e])


class GenotypeResult:
    """Per event e: gl[e] / pl[e] as [n_samples, G_e] arrays (genotypes in index order), n_evidence[e] per sample."""

    def __init__(self, gl, pl, n_evidence):
        self.gl, self.pl, self.n_evidence = gl, pl, n_evidence


def genotype_likelihoods(engine, batch, likelihoods, keep, read_start, read_end_, read_sample, events, ploidy=2, n_samples=1):
    """`likelihoods`: the per-region [read][hap] matrices at batch.out_off (phmm_engine_compute / phmm_region_compute);
    `keep`: their evidence flags (or None: every read); read_start / read_end_: each read's closed span on the reference
    after realignment (read_end); read_sample: each read's sample; events: Events."""
    lk = np.ascontiguousarray(likelihoods, np.float64)
    kp = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    rs, re_ = np.ascontiguousarray(read_start, np.int64), np.ascontiguousarray(read_end_, np.int64)
    smp = np.ascontiguousarray(read_sample, np.uint32)
    n_ev = events.n_events
    G = np.array([genotype_count(ploidy, events.n_alleles(e)) for e in range(n_ev)], np.uint64)
    gl_off = np.concatenate([[0], np.cumsum(G * np.uint64(n_samples))]).astype(np.uint64)
    gl, pl = np.zeros(int(gl_off[-1])), np.zeros(int(gl_off[-1]), np.int32)
    n_evidence = np.zeros(n_ev * n_samples, np.uint32)
    code = engine.lib.phmm_genotype_likelihoods(
        engine._h, batch.n_regions, _p(batch.region_read_off, _lib.u32p), _p(batch.region_hap_off, _lib.u32p), _p(batch.out_off, _lib.u64p),
        _p(lk, _lib.f64p), _p(kp, _lib.u8p), _p(smp, _lib.u32p), _p(rs, _i64p), _p(re_, _i64p), int(n_samples), int(ploidy), n_ev,
        _p(events.region, _lib.u32p), _p(events.allele_off, _lib.u32p), _p(events.start, _i64p), _p(events.end, _i64p),
        _p(events.hap_allele, _i32p), _p(gl_off, _lib.u64p), _p(gl, _lib.f64p), _p(pl, _i32p), _p(n_evidence, _lib.u32p))
    if code != _lib.PHMM_OK:
        raise PhmmError(code, engine.last_error())
    shape = lambda e: (int(n_samples), int(G[e]))  # noqa: E731
    return GenotypeResult([gl[int(gl_off[e]):int(gl_off[e + 1])].reshape(shape(e)) for e in range(n_ev)],
                          [pl[int(gl_off[e]):int(gl_off[e + 1])].reshape(shape(e)) for e in range(n_ev)],
                          n_evidence.reshape(n_ev, int(n_samples)))


# ---- the allele-frequency calculation (phmm_allele_frequency) ------------------------------------------------------------

def pseudo_counts(snp_het=0.001, indel_het=0.000125, het_stdev=0.01):
    """(ref, snp, indel) pseudo counts as AlleleFrequencyCalculator::make_calculator makes them
    (src/model/allele_frequency_calculator.rs:53-75) from --snp-heterozygosity, --indel-heterozygosity and
    --heterozygosity-stdev (defaults: src/cli.rs:1509-1526)."""
    ref = snp_het / (het_stdev ** 2.0)
    return ref, snp_het * ref, indel_het * ref


class AFResult:
    """Per event e: log10_p_no_variant[e], log10_p_variant_present[e], qual[e], flags[e] (PHMM_AF_*), iterations[e];
    per event the arrays over its alleles (reference first): log10_p_absent[e] (reference slot 0.0), mle_count[e],
    allele_flags[e] (PHMM_AF_ALLELE_*)."""

    def __init__(self, allele_off, pnv, pvp, absent, mle, aflags, qual, flags, iterations):
        self.log10_p_no_variant, self.log10_p_variant_present, self.qual = pnv, pvp, qual
        self.flags, self.iterations = flags, iterations
        cut = lambda a: [a[int(allele_off[e]):int(allele_off[e + 1])] for e in range(len(allele_off) - 1)]  # noqa: E731
        self.log10_p_absent, self.mle_count, self.allele_flags = cut(absent), cut(mle), cut(aflags)

    def called(self, e):
        return bool(self.flags[e] & _lib.PHMM_AF_CALLED)


def allele_frequency(engine, pl, pl_off=None, allele_off=None, allele_length=None, allele_kind=None, n_samples=1, ploidy=2,
                     pseudo_counts=pseudo_counts(), stand_min_conf=30.0):
    """The allele-frequency step of calculate_genotypes for a batch of events (phmm_allele_frequency, include/phmm.h).
    `pl`: the PLs, flat with pl_off [n_events + 1] (n_samples x G_e per event, sample-major), or a GenotypeResult of
    genotype_likelihoods (pl_off then comes from it); allele_off [n_events + 1]; allele_length: Allele::length() per allele;
    allele_kind: PHMM_AF_KIND_* per allele or None (all plain); pseudo_counts: (ref, snp, indel)."""
    if isinstance(pl, GenotypeResult):
        n_samples = np.shape(pl.pl[0])[0] if pl.pl else n_samples
        parts = [np.ascontiguousarray(x, np.int32).reshape(-1) for x in pl.pl]
        pl_off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64)
        pl = np.concatenate(parts) if parts else np.zeros(0, np.int32)
    pl = np.ascontiguousarray(pl, np.int32)
    pl_off = np.ascontiguousarray(pl_off, np.uint64)
    ao = np.ascontiguousarray(allele_off, np.uint32)
    ln = np.ascontiguousarray(allele_length, np.uint32)
    kd = None if allele_kind is None else np.ascontiguousarray(allele_kind, np.uint8)
    n_ev, n_al = len(ao) - 1, int(ao[-1]) if len(ao) else 0
    pnv, pvp, qual = np.zeros(n_ev), np.zeros(n_ev), np.zeros(n_ev)
    flags, iters = np.zeros(n_ev, np.uint32), np.zeros(n_ev, np.uint32)
    absent, mle, aflags = np.zeros(n_al), np.zeros(n_al, np.int64), np.zeros(n_al, np.uint8)
    ref, snp, indel = (float(x) for x in pseudo_counts)
    code = engine.lib.phmm_allele_frequency(
        engine._h, n_ev, int(n_samples), int(ploidy), _p(ao, _lib.u32p), _p(ln, _lib.u32p), _p(kd, _lib.u8p), _p(pl_off, _lib.u64p),
        _p(pl, _i32p), ref, snp, indel, float(stand_min_conf), _p(pnv, _lib.f64p), _p(pvp, _lib.f64p), _p(absent, _lib.f64p),
        _p(mle, _i64p), _p(aflags, _lib.u8p), _p(qual, _lib.f64p), _p(flags, _lib.u32p), _p(iters, _lib.u32p))
    if code != _lib.PHMM_OK:
        raise PhmmError(code, engine.last_error())
    return AFResult(ao, pnv, pvp, absent, mle, aflags, qual, flags, iters)


# ---- genotype assignment (phmm_assign_genotypes) ---------------------------------------------------------------------------

class AssignResult:
    """Per event e: sub_pl[e] as an [n_samples, G'_e] array over the genotypes of the call's alleles (gp[e] / pg[e] alike with
    the posterior method, else None); gt as [n_events, n_samples, ploidy] indices into the call's alleles (-1: no call); gq
    (-1: none), log10_gq, sample_called, sample_flags (PHMM_GT_SAMPLE_*) as [n_events, n_samples];
    log10_p_error_posterior per event (posterior method; NaN: no update) or None; call_alleles as given."""

    def __init__(self, call_alleles, sub_pl, gt, gq, log10_gq, sample_called, sample_flags, gp, pg, log10_p_error_posterior):
        self.call_alleles, self.sub_pl, self.gt, self.gq, self.log10_gq = call_alleles, sub_pl, gt, gq, log10_gq
        self.sample_called, self.sample_flags, self.gp, self.pg = sample_called, sample_flags, gp, pg
        self.log10_p_error_posterior = log10_p_error_posterior


def assign_genotypes(engine, af_or_call_alleles, pl, allele_off, pl_off=None, allele_length=None, allele_kind=None,
                     n_samples=1, ploidy=2, method=_lib.PHMM_GT_USE_PLS, log10_snp_het=-3.0, log10_indel_het=np.log10(1.25e-4),
                     site_monomorphic=None):
    """PL subsetting, GT and GQ per sample for a batch of events (phmm_assign_genotypes, include/phmm.h).
    af_or_call_alleles: an AFResult of allele_frequency (the call's alleles and site_monomorphic then come from it) or per
    event the indices of the call's alleles (reference first; empty: not called); pl / pl_off / allele_length / allele_kind: as
    allele_frequency takes them (pl_off comes from a GenotypeResult, else it is required); allele_off [n_events + 1]; log10_snp_het / log10_indel_het: log10 of --snp-heterozygosity and
    --indel-heterozygosity (defaults: src/cli.rs:1509-1520), the posterior method's."""
    if isinstance(af_or_call_alleles, AFResult):
        call_alleles = call_alleles_of(af_or_call_alleles)
        if site_monomorphic is None:
            site_monomorphic = (np.asarray(af_or_call_alleles.flags) & _lib.PHMM_AF_MONOMORPHIC) != 0
    else:
        call_alleles = [list(c) for c in af_or_call_alleles]
    if isinstance(pl, GenotypeResult):
        n_samples = np.shape(pl.pl[0])[0] if pl.pl else n_samples
        parts = [np.ascontiguousarray(x, np.int32).reshape(-1) for x in pl.pl]
        pl_off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint64)
        pl = np.concatenate(parts) if parts else np.zeros(0, np.int32)
    if pl_off is None:
        raise ValueError("assign_genotypes: pl_off is required unless pl is a GenotypeResult")
    pl = np.ascontiguousarray(pl, np.int32)
    pl_off = np.ascontiguousarray(pl_off, np.uint64)
    ao = np.ascontiguousarray(allele_off, np.uint32)
    ln = None if allele_length is None else np.ascontiguousarray(allele_length, np.uint32)
    kd = None if allele_kind is None else np.ascontiguousarray(allele_kind, np.uint8)
    mono = None if site_monomorphic is None else np.ascontiguousarray(site_monomorphic, np.uint8)
    n_ev, S, P = len(ao) - 1, int(n_samples), int(ploidy)
    C = np.array([len(c) for c in call_alleles], np.int64)
    c_off = np.concatenate([[0], np.cumsum(C)]).astype(np.uint32)
    ca = np.array([a for c in call_alleles for a in c] + ([] if int(c_off[-1]) else [0]), np.uint32)
    Gn = np.array([genotype_count(P, int(c)) if c >= 2 else 0 for c in C], np.uint64)
    s_off = np.concatenate([[0], np.cumsum(Gn * np.uint64(S))]).astype(np.uint64)
    n_sub = max(int(s_off[-1]), 1)
    posterior = int(method) == _lib.PHMM_GT_USE_POSTERIORS
    sub_pl, gt = np.zeros(n_sub, np.int32), np.zeros(max(n_ev * S * P, 1), np.int32)
    gq, log10_gq = np.zeros(n_ev * S, np.int32), np.zeros(n_ev * S)
    called, sflags = np.zeros(n_ev * S, np.uint8), np.zeros(n_ev * S, np.uint8)
    gp, pg, upd = (np.zeros(n_sub), np.zeros(n_sub), np.zeros(n_ev)) if posterior else (None, None, None)
    code = engine.lib.phmm_assign_genotypes(
        engine._h, n_ev, S, P, _p(ao, _lib.u32p), _p(ln, _lib.u32p), _p(kd, _lib.u8p), _p(pl_off, _lib.u64p), _p(pl, _i32p),
        _p(c_off, _lib.u32p), _p(ca, _lib.u32p), int(method), float(log10_snp_het), float(log10_indel_het), _p(mono, _lib.u8p),
        _p(s_off, _lib.u64p), _p(sub_pl, _i32p), _p(gt, _i32p), _p(gq, _i32p), _p(log10_gq, _lib.f64p), _p(called, _lib.u8p),
        _p(sflags, _lib.u8p), _p(gp, _lib.f64p), _p(pg, _lib.f64p), _p(upd, _lib.f64p))
    if code != _lib.PHMM_OK:
        raise PhmmError(code, engine.last_error())
    cut = lambda a: None if a is None else [a[int(s_off[e]):int(s_off[e + 1])].reshape(S, int(Gn[e])) for e in range(n_ev)]  # noqa: E731
    return AssignResult(call_alleles, cut(sub_pl), gt[:n_ev * S * P].reshape(n_ev, S, P), gq.reshape(n_ev, S), log10_gq.reshape(n_ev, S),
                        called.reshape(n_ev, S), sflags.reshape(n_ev, S), cut(gp), cut(pg), upd)


# ---- the annotation of called events (phmm_annotate_events) ----------------------------------------------------------------

class AlignedReads:
    """What BQ reads of each evidence read (all reads of the batch, in order): read_off [n_reads + 1] into base_q, the read's
    CIGAR after realignment (BAM-encoded elements; `cigars`: one array per read), its soft start, and per event its position
    (vc.loc.start)."""

    def __init__(self, read_off, base_q, cigars, soft_start, event_pos):
        self.read_off = np.ascontiguousarray(read_off, np.uint32)
        self.base_q = np.ascontiguousarray(base_q, np.uint8)
        cigars = [np.ascontiguousarray(c, np.uint32) for c in cigars]
        self.n_cigar = np.array([len(c) for c in cigars], np.uint32)
        self.cigar_off = np.concatenate([[0], np.cumsum(self.n_cigar)]).astype(np.uint64)
        self.cigar = np.concatenate(cigars).astype(np.uint32) if cigars else np.zeros(0, np.uint32)
        if not len(self.cigar):
            self.cigar = np.zeros(1, np.uint32)
        self.soft_start = np.ascontiguousarray(soft_start, np.int64)
        self.event_pos = np.ascontiguousarray(event_pos, np.int64)


class AnnotationResult:
    """Per event e: ad[e] / af[e] as [n_samples, C_e] arrays, mq[e] / bq[e] over its call alleles (bq None without the BQ
    inputs); dp / ac as [n_events, n_samples]; info_dp, qd_depth, qd, flags (PHMM_ANN_*) per event."""

    def __init__(self, ad, af, dp, ac, mq, bq, info_dp, qd_depth, qd, flags):
        self.ad, self.af, self.dp, self.ac, self.mq, self.bq = ad, af, dp, ac, mq, bq
        self.info_dp, self.qd_depth, self.qd, self.flags = info_dp, qd_depth, qd, flags


def call_alleles_of(af_result):
    """The alleles of each call from an AFResult: the reference and every allele with PHMM_AF_ALLELE_OUTPUT, for the events
    that are CALLED; an empty list otherwise."""
    return [[0] + [a for a in range(1, len(fl)) if fl[a] & _lib.PHMM_AF_ALLELE_OUTPUT] if af_result.called(e) else []
            for e, fl in enumerate(af_result.allele_flags)]


def annotate_events(engine, batch, likelihoods, keep, read_start, read_end_, read_sample, mapq, events, call_alleles,
                    log10_p_error, n_samples=1, aligned=None, sample_called=None, n_filtered=None):
    """AD, DP, AF, AC per sample and DP, QD, MQ, BQ per event for a batch of called events (phmm_annotate_events,
    include/phmm.h).  The region / read / event arguments are genotype_likelihoods'; mapq: per read; call_alleles: per event
    the indices of the call's alleles among the event's (reference first; empty: not annotated; call_alleles_of);
    log10_p_error: per event (NaN: none); aligned: AlignedReads or None (no BQ); sample_called: [n_events, n_samples], an
    AssignResult of assign_genotypes (its sample_called) or None; n_filtered: [n_events, n_samples] or None."""
    if isinstance(sample_called, AssignResult):
        sample_called = sample_called.sample_called
    lk = np.ascontiguousarray(likelihoods, np.float64)
    kp = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    rs, re_ = np.ascontiguousarray(read_start, np.int64), np.ascontiguousarray(read_end_, np.int64)
    smp, mq_in = np.ascontiguousarray(read_sample, np.uint32), np.ascontiguousarray(mapq, np.uint8)
    n_ev, S = events.n_events, int(n_samples)
    C = np.array([len(c) for c in call_alleles], np.int64)
    c_off = np.concatenate([[0], np.cumsum(C)]).astype(np.uint32)
    ca = np.array([a for c in call_alleles for a in c] + ([] if int(c_off[-1]) else [0]), np.uint32)
    err = np.ascontiguousarray(log10_p_error, np.float64)
    sc = None if sample_called is None else np.ascontiguousarray(sample_called, np.uint8).reshape(-1)
    nf = None if n_filtered is None else np.ascontiguousarray(n_filtered, np.uint32).reshape(-1)
    n_call = int(c_off[-1])
    ad, af = np.zeros(n_call * S, np.int32), np.zeros(n_call * S)
    dp, ac = np.zeros(n_ev * S, np.int32), np.zeros(n_ev * S, np.uint32)
    mq, bq = np.zeros(n_call, np.uint8), None if aligned is None else np.zeros(n_call, np.uint8)
    info_dp, qd_depth, qd, flags = np.zeros(n_ev, np.int32), np.zeros(n_ev, np.int32), np.zeros(n_ev), np.zeros(n_ev, np.uint32)
    al = aligned
    code = engine.lib.phmm_annotate_events(
        engine._h, batch.n_regions, _p(batch.region_read_off, _lib.u32p), _p(batch.region_hap_off, _lib.u32p), _p(batch.out_off, _lib.u64p),
        _p(lk, _lib.f64p), _p(kp, _lib.u8p), _p(smp, _lib.u32p), _p(rs, _i64p), _p(re_, _i64p), _p(mq_in, _lib.u8p), S, n_ev,
        _p(events.region, _lib.u32p), _p(events.allele_off, _lib.u32p), _p(events.start, _i64p), _p(events.end, _i64p),
        _p(events.hap_allele, _i32p), _p(c_off, _lib.u32p), _p(ca, _lib.u32p),
        _p(al and al.read_off, _lib.u32p), _p(al and al.base_q, _lib.u8p), _p(al and al.cigar_off, _lib.u64p), _p(al and al.cigar, _lib.u32p),
        _p(al and al.n_cigar, _lib.u32p), _p(al and al.soft_start, _i64p), _p(al and al.event_pos, _i64p),
        _p(sc, _lib.u8p), _p(err, _lib.f64p), _p(nf, _lib.u32p), _p(ad, _i32p), _p(dp, _i32p), _p(af, _lib.f64p), _p(ac, _lib.u32p),
        _p(mq, _lib.u8p), _p(bq, _lib.u8p), _p(info_dp, _i32p), _p(qd_depth, _i32p), _p(qd, _lib.f64p), _p(flags, _lib.u32p))
    if code != _lib.PHMM_OK:
        raise PhmmError(code, engine.last_error())
    lo = lambda e: int(c_off[e])  # noqa: E731
    per_sample = lambda a: [a[S * lo(e):S * lo(e + 1)].reshape(S, int(C[e])) for e in range(n_ev)]  # noqa: E731
    per_allele = lambda a: None if a is None else [a[lo(e):lo(e + 1)] for e in range(n_ev)]  # noqa: E731
    return AnnotationResult(per_sample(ad), per_sample(af), dp.reshape(n_ev, S), ac.reshape(n_ev, S), per_allele(mq), per_allele(bq),
                            info_dp, qd_depth, qd, flags)
