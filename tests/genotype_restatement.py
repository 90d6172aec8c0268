"""Test infrastructure, not product code: a statement-by-statement restatement of the reference's genotyping step for one
region's events, what tests/test_genotype_hip.py holds the device to bit for bit.

  marginalize       AlleleLikelihoods::marginal_likelihoods (src/model/allele_likelihoods.rs:693-740)
  retain_evidence   the genotyping predicate (src/haplotype/haplotype_caller_genotyping_engine.rs:759-768) with
                    Locatable::overlaps (src/utils/simple_interval.rs:298-307)
  genotypes         build_allele_first_genotype_offset_table (src/genotype/genotype_likelihood_calculators.rs:180-200),
                    allele_heap_to_index (src/genotype/genotype_likelihood_calculator.rs:273-295)
  GL                genotype_likelihoods (genotype_likelihood_calculator.rs:308-580)
  PL                GenotypeLikelihoods::gls_to_pls / max_pl (src/genotype/genotype_likelihoods.rs:55-78)

The JacobianLogTable sums come from the oracle (oracle_approximate_log10_sum_log10): table[k] = f(-k * 1e-4, 0.0), the
last entry through a difference just under MAX_TOLERANCE.  Vectorised over reads without changing the semantics: rounding
half away from zero, sequential sums (np.add.accumulate), INV_STEP computed as 1.0 / 0.0001."""
import functools
import itertools
import math

import numpy as np

from oracle import oracle

MAX_TOLERANCE = 8.0      # math_utils.rs:485
TABLE_STEP = 0.0001      # math_utils.rs:490
INV_STEP = 1.0 / TABLE_STEP
I32_MAX = 2 ** 31 - 1
_TABLE = None


def jacobian_table():
    global _TABLE
    if _TABLE is None:
        f = oracle.lib().oracle_approximate_log10_sum_log10
        n = int((MAX_TOLERANCE / TABLE_STEP) + 1.0)
        t = np.array([f(-k * TABLE_STEP, 0.0) for k in range(n - 1)] + [f(-7.99996, 0.0)])
        _TABLE = t
    return _TABLE


def round_half_away(x):
    """f64::round (numpy's np.round rounds half to even)."""
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    fl = np.floor(a)
    r = np.where(a - fl >= 0.5, fl + 1.0, fl)
    return np.copysign(r, x)


def _get(diff):
    """JacobianLogTable::get: cache[(diff * INV_STEP).round() as usize] (diff >= 0 wherever it is called)."""
    return jacobian_table()[round_half_away(diff * INV_STEP).astype(np.int64)]


def approximate_log10_sum_log10(a, b):
    """math_utils.rs:314-332, element-wise."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    lo, hi = np.where(a > b, b, a), np.where(a > b, a, b)
    with np.errstate(invalid="ignore"):
        diff = hi - lo
    inside = (lo != -np.inf) & (diff < MAX_TOLERANCE)
    corr = np.zeros_like(hi)
    corr[inside] = _get(diff[inside])
    return np.where(lo == -np.inf, hi, hi + corr)


def approximate_log10_sum_log10_vec(vals):
    """math_utils.rs:344-370 over axis 0 of vals [components, reads]: from the first maximal element, the others in order."""
    vals = np.asarray(vals, np.float64)
    n = vals.shape[1]
    imax = np.zeros(n, np.int64)
    for c in range(1, vals.shape[0]):  # max_element_index: strictly greater replaces
        imax = np.where(vals[c] > vals[imax, np.arange(n)], c, imax)
    s = vals[imax, np.arange(n)].copy()
    for c in range(vals.shape[0]):
        v = vals[c]
        go = (imax != c) & (v != -np.inf)
        with np.errstate(invalid="ignore"):
            diff = s - v
        go &= diff < MAX_TOLERANCE
        s[go] = s[go] + _get(diff[go])
    return s


def offset_table(ploidy, allele_count):
    """build_allele_first_genotype_offset_table (genotype_likelihood_calculators.rs:180-200)."""
    t = np.zeros((ploidy + 1, allele_count + 1), np.int64)
    t[0, 1:] = 1
    for p in range(1, ploidy + 1):
        for a in range(1, allele_count + 1):
            t[p, a] = t[p, a - 1] + t[p - 1, a]
    return t


def alleles_to_index(alleles, offsets):
    """allele_heap_to_index: pop the largest allele with ploidy p, p - 1, ..."""
    heap = sorted(alleles)
    result = 0
    for p in range(len(heap), 0, -1):
        result += int(offsets[p, heap.pop()])
    return result


def genotype_count(ploidy, allele_count):
    """calculate_genotype_count (tests/genotype_likelihood_calculator_unit_tests.rs:162-175), iteratively."""
    if ploidy == 0:
        return 0
    row = [a for a in range(allele_count + 1)]  # ploidy 1
    for _ in range(2, ploidy + 1):
        nxt = [0] * (allele_count + 1)
        for a in range(1, allele_count + 1):
            nxt[a] = row[a] + nxt[a - 1]
        row = nxt
    return row[allele_count]


@functools.lru_cache(maxsize=None)
def genotypes(ploidy, allele_count):
    """Every genotype as (alleles ascending, counts), in index order."""
    off = offset_table(ploidy, allele_count)
    out = [None] * int(off[ploidy, allele_count])
    for al in itertools.combinations_with_replacement(range(allele_count), ploidy):
        distinct = sorted(set(al))
        out[alleles_to_index(list(al), off)] = (distinct, [al.count(a) for a in distinct])
    return out


def overlaps(w0, w1, start, end):
    """Locatable::overlaps with the window as self and the read as other."""
    return ((start >= w0) & (start <= w1)) | ((end >= w0) & (end <= w1)) | ((w0 >= start) & (w1 <= end))


def marginalize(L, hap_allele, n_alleles):
    """L [reads, haps] -> M [alleles, reads]: max over the haplotypes of each allele, from -inf, strictly greater replaces."""
    M = np.full((n_alleles, L.shape[0]), -np.inf)
    for h, a in enumerate(hap_allele):
        if a < 0:
            continue
        v = L[:, h]
        M[a] = np.where(v > M[a], v, M[a])
    return M


def genotype_likelihoods_of(M, ploidy):
    """GenotypeLikelihoodCalculator::genotype_likelihoods on the used reads' marginals M [alleles, reads] -> GL [G]."""
    n = M.shape[1]
    comp = lambda a, c: M[a] if c == 1 else M[a] + math.log10(c)  # noqa: E731  (frequency-c row, :606-660)
    gts = genotypes(ploidy, M.shape[0])
    per_read = np.zeros((len(gts), n))
    for g, (al, cn) in enumerate(gts):
        if n == 0:
            continue
        if len(al) == 1:
            per_read[g] = comp(al[0], cn[0])
        elif len(al) == 2:
            per_read[g] = approximate_log10_sum_log10(comp(al[0], cn[0]), comp(al[1], ploidy - cn[0]))
        else:
            per_read[g] = approximate_log10_sum_log10_vec(np.stack([comp(a, c) for a, c in zip(al, cn)]))
    sums = np.add.accumulate(np.concatenate([np.zeros((len(gts), 1)), per_read], axis=1), axis=1)[:, -1]
    return sums - float(n) * math.log10(float(ploidy))


def gls_to_pls(gl):
    adjust = -np.inf
    for x in gl:  # max(OrderedFloat(adjust), OrderedFloat(x))
        adjust = x if not (x < adjust) else adjust
    with np.errstate(invalid="ignore"):
        v = round_half_away(-10.0 * (np.asarray(gl) - adjust))
    out = np.where(np.isnan(v), 0, np.clip(np.nan_to_num(v, nan=0.0, posinf=I32_MAX, neginf=-I32_MAX - 1), -I32_MAX - 1, I32_MAX))
    return np.minimum(out.astype(np.int64), I32_MAX).astype(np.int32)


def region_events(L, keep, read_sample, read_start, read_end, n_samples, ploidy, events):
    """One region's matrix L [reads, haps] and its events [(n_alleles, hap_allele, w0, w1)] ->
    per event (GL [n_samples, G], PL [n_samples, G], n_evidence [n_samples])."""
    out = []
    keep = np.ones(L.shape[0], bool) if keep is None else np.asarray(keep) != 0
    for n_alleles, hap_allele, w0, w1 in events:
        M_all = marginalize(L, hap_allele, n_alleles)
        gl, pl, ne = [], [], []
        for s in range(n_samples):
            used = np.flatnonzero(keep & (read_sample == s) & overlaps(w0, w1, read_start, read_end))
            g = genotype_likelihoods_of(M_all[:, used], ploidy)
            gl.append(g)
            pl.append(gls_to_pls(g))
            ne.append(len(used))
        out.append((np.array(gl), np.array(pl), np.array(ne, np.uint32)))
    return out


def batch_events(batch, likelihoods, keep, read_sample, read_start, read_end, n_samples, ploidy, ev, only=None):
    """region_events over a RegionBatch and a genotype.Events; `only`: the event indices to restate (default all)."""
    res = {}
    nh_of = np.diff(batch.region_hap_off.astype(np.int64))[ev.region.astype(np.int64)]
    map_off = np.concatenate([[0], np.cumsum(nh_of)])
    for e in (range(ev.n_events) if only is None else only):
        g = int(ev.region[e])
        r0, r1 = int(batch.region_read_off[g]), int(batch.region_read_off[g + 1])
        nh = int(batch.region_hap_off[g + 1] - batch.region_hap_off[g])
        L = np.asarray(likelihoods[int(batch.out_off[g]):int(batch.out_off[g]) + (r1 - r0) * nh]).reshape(r1 - r0, nh)
        moff = int(map_off[e])
        kp = None if keep is None else keep[r0:r1]
        res[e] = region_events(L, kp, read_sample[r0:r1], read_start[r0:r1], read_end[r0:r1], n_samples, ploidy,
                               [(ev.n_alleles(e), ev.hap_allele[moff:moff + nh], int(ev.start[e]), int(ev.end[e]))])[0]
    return res
