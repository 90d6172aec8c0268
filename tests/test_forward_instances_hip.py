"""Every compiled instance of the PairHMM forward kernels against the oracle, each at the haplotype lengths that select it:
  per read     phmm_forward<L,K>            L in 16, 32, 64 x K = 2 ... 32          93 instances, a small launch (the v_cndmask
                                                                                      body for K <= 13) and one of 4 160 reads
                                                                                      (the EXEC body, no split over gridDim.y)
  chained f64  phmm_forward_chain<L,K>      L in 16, 32, 64 x K = 2 ... 25          72, at 16 lanes with the planner's streams and
                                                                                      with 1, 2 and 4 forced; runs of 64 once per L
  range        phmm_forward_chain<L,LO,HI>  L x the four ranges of K                12 mixed launches
  chained f32  phmm_forward_chain_f32<L,K>  L in 16, 32 x K = 2 ... 25              48, 1 / 2 / 4 streams at 16 lanes,
               phmm_forward_chain_f32_any<L>                                         and the any-K kernel of both lane counts
and a sweep of the f32 trust line (likelihood x haplotype length = 2^-196 ~ 1e-59, phmm_chain32_kernels.hip) like the one
test_underflow_band.py has for the bottom of the f64 range.  After planning, the plan must name the instance the case is for.

f64 results: test_hip_parity._close at its TOL_VS_ORACLE.  f32 results: within test_f32_first.TOL_F32 of the oracle, never
NaN, never positive; reads the f32 kernel hands over are the f64 per-read kernel's results bit for bit.

The builders are plain numpy (no GPU needed to import them): tests/test_forward_instance_table.py holds the tables against
the kernel sources, the batches against the planner (phmm_plan_describe) and the inputs against the oracle.

Cost: the oracle is asked for 3.9e9 cells by this file: 0.24e9 for the 93 instance batches (computed once, shared by the
per-read, the chained and the f32 cases), 3.33e9 for the 93 launches of 4 160 short reads, 0.09e9 for the range, any-K and
run-of-64 batches, 0.22e9 for the trust line's pools and bands.  (Short reads cost the oracle more per cell than long ones:
its set-up per pair; the 93 large launches are most of this file's time.)"""
import re
import zlib

import numpy as np
import pytest

from lorikeet_amd.batch import RegionBatch
from oracle import oracle
from test_f32_first import TOL_F32                   # 1e-5: the reference's own gate for its vector path
from test_hip_parity import TOL_VS_ORACLE, _close    # 1e-9

LANES = (16, 32, 64)
FORWARD_K = tuple(range(2, 33))          # PHMM_K_LIST / kInstantiatedK
CHAIN_K = tuple(range(2, 26))            # PHMM_CHAIN_K_LIST, chain_max_k()
CHAIN_LANES = (16, 32, 64)               # -DPHMM_CHAIN_L
CHAIN32_K = tuple(range(2, 26))          # PHMM_CHAIN32_K_LIST
CHAIN32_LANES = (16, 32)                 # -DPHMM_CHAIN32_L
CHAIN_RANGES = ((2, 9), (10, 15), (16, 19), (20, 25))   # PHMM_CHAIN_RANGES
SDWA_MIN_K, CND_MAX_K, TWO_WAVE_MAX_K = 21, 13, 25      # phmm_device.hpp
NUM_SIMD = 1024                          # phmm_plan.hpp, kNumSimd
CHAIN_MAX_READS = 64
RUN = 5                                  # forced run length: divides none of the read counts below

ALPHA = np.frombuffer(b"ACGT", np.uint8)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _rnd(rng, n):
    return ALPHA[rng.integers(0, 4, n)]


# ---- reads and haplotypes -------------------------------------------------------------------------------------------------
LONG = 70   # reads above this get gap-continuation penalties of 1 ... 10 (see _quals)


def _quals(rng, n):
    """(base quality, insertion, deletion, gcp).  Base quality and gcp >= 1 (the fast path), insertion / deletion >= 6 (below Q4
    the transition model is improper, test_hip_parity._random_region); everything up to 60 -- except the gcp of reads longer
    than LONG rows, which stays below 11: a read that cannot follow its haplotype (unrelated, or longer than it) then pays
    about 0.55 per row as one insertion instead of 3, and stays above 1e-300 -- the numbers are the instance's, not phmm_rescue's."""
    gmax = 61 if n <= LONG else 11
    return (rng.integers(1, 61, n).astype(np.uint8), rng.integers(6, 61, n).astype(np.uint8), rng.integers(6, 61, n).astype(np.uint8),
            rng.integers(1, gmax, n).astype(np.uint8))


def _read(rng, n, root, related):
    """A read of n rows: unrelated, or a window of `root` with substitutions and (from 24 rows) one two-base insertion or deletion."""
    if not related or len(root) == 0:
        return (_rnd(rng, n),) + _quals(rng, n)
    s = int(rng.integers(0, max(1, len(root) - n + 1)))
    seg = root[s:s + n + 2]
    if n >= 24:
        cut = n // 2
        if rng.random() < 0.5:
            seg = np.concatenate([seg[:cut], seg[cut + 2:]])            # two bases of the haplotype missing from the read
        else:
            seg = np.concatenate([seg[:cut], _rnd(rng, 2), seg[cut:]])  # two bases more than the haplotype has
    seg = seg[:n]
    if len(seg) < n:
        seg = np.concatenate([seg, _rnd(rng, n - len(seg))])
    seg = seg.copy()
    hit = rng.random(n) < 0.03
    seg[hit] = ALPHA[(np.searchsorted(ALPHA, seg[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4]
    return (seg,) + _quals(rng, n)


def _hap(rng, root, length):
    """The first `length` bases of `root`, two of them substituted from eight bases on."""
    h = root[:length].copy()
    if length >= 8:
        h[rng.integers(0, length, 2)] = _rnd(rng, 2)
    return h


def boundary_lengths(L, K):
    """The longest haplotypes of a region that selects K: one column in the last lane in use ... the last column empty, all full."""
    return (L * (K - 1) + 1, L * K - 1, L * K)


def short_lengths(L, K):
    """The other haplotypes: 1; one lane, one lane plus a column; half the lanes idle; multiples of K (the edge column is a lane's last)."""
    return (1, K, K + 1, (L * K) // 2, K * (L // 4), 3 * K)


def hap_counts(L):
    """1, the wave's slots filled exactly, one more (a second group with idle slots), and nine at 16 lanes."""
    G = 64 // L
    return (1, G, G + 1) + ((9,) if L == 16 else ())


def _to_batch(regions):
    """[(reads, haplotypes)] with reads = (bases, base quality, insertion, deletion, gcp) -> RegionBatch."""
    rro, rho, ro, ho, oo = [0], [0], [0], [0], [0]
    cols, hb = [[], [], [], [], []], []
    for reads, haps in regions:
        for rd in reads:
            for c, a in zip(cols, rd):
                c.append(a)
            ro.append(ro[-1] + len(rd[0]))
        for h in haps:
            hb.append(h)
            ho.append(ho[-1] + len(h))
        rro.append(rro[-1] + len(reads))
        rho.append(rho[-1] + len(haps))
        oo.append(oo[-1] + len(reads) * len(haps))
    cat = lambda xs: np.ascontiguousarray(np.concatenate(xs), dtype=np.uint8)  # noqa: E731
    return RegionBatch(region_read_off=np.asarray(rro, np.uint32), region_hap_off=np.asarray(rho, np.uint32),
                       read_off=np.asarray(ro, np.uint32), hap_off=np.asarray(ho, np.uint32), out_off=np.asarray(oo, np.uint64),
                       read_bases=cat(cols[0]), base_q=cat(cols[1]), ins_q=cat(cols[2]), del_q=cat(cols[3]), gcp=cat(cols[4]),
                       hap_bases=cat(hb))


# read counts of the regions: none a multiple of RUN (short last runs, 11 = 5 + 5 + 1: a run of one read), 1 and 3 reads (fewer
# than two / four streams), and the rows of the reads.  "general": one haplotype has an 'N', one read a gcp == 0, one a base
# quality 0 -- ROW_GENERAL per read, the in-wave general path chained, the wholesale hand-over of the f32 kernels.
def _region_plan(L):
    G = 64 // L
    sm = [1, 2, L - 1, L, L + 1]
    plan = [
        dict(nh=1, longest=2, rows=sm + [30, 47, 8, 23, 61, 12]),
        dict(nh=G, longest=1, rows=[L, 1, 40, L + 1, 19, 2, 55]),
        dict(nh=G + 1, longest=0, rows=sm + [33, 64, 9, 27, 45, 16, 70, 5]),
        dict(nh=G + 1, longest=2, rows=[20, L, 31, 7, L + 1, 44, 13, 58], general=True),
        dict(nh=max(2, G), longest=1, rows=[26, 3, L - 1, 39, 52, 10], general=True),
        dict(nh=2, longest=2, rows=[37]),
        dict(nh=1, longest=0, rows=[L, 29, 1]),
        dict(nh=max(3, G + 1), longest=2, rows=[150, 300, L, 151, 1, 149], also=(1, 0)),   # 300 rows: past lds_rows = 256, round the ring
    ]
    if L == 16:
        plan.insert(3, dict(nh=9, longest=2, rows=[L - 1, 50, 2, 35, L + 1, 66, 11, 24, 42]))
    return plan


def instance_regions(L, K):
    """The regions of instance <L, K> -> [(reads, haplotypes, general)]; the same bytes every time."""
    rng = _rng("instance", L, K)
    bl, sl = boundary_lengths(L, K), short_lengths(L, K)
    si = 0
    out = []
    for spec in _region_plan(L):
        root = _rnd(rng, L * K)
        lens = [bl[spec["longest"]]] + [bl[i] for i in spec.get("also", ())][:spec["nh"] - 1]
        while len(lens) < spec["nh"]:
            lens.append(sl[si % len(sl)])
            si += 1
        haps = [_hap(rng, root, n) for n in lens]
        reads = [_read(rng, n, root, related=(i % 3 != 2)) for i, n in enumerate(spec["rows"])]
        if spec.get("general"):
            haps[-1 if spec["nh"] > 1 else 0][lens[-1 if spec["nh"] > 1 else 0] // 2] = ord("N")
            # gcp == 0: no way out of that row's deletion state but into the next row's match state at its full weight again --
            # along a haplotype of a thousand columns an improper model that the reference refuses (result > 0) unless the way
            # into the state is narrow: deletion quality 60 on that row
            reads[1][4][len(reads[1][4]) // 2] = 0
            reads[1][3][len(reads[1][4]) // 2] = 60
            reads[3][1][len(reads[3][1]) // 3] = 0     # base quality 0: match prior 0
        out.append((reads, haps, bool(spec.get("general"))))
    return out


def _batch_of(regions):
    b = _to_batch([(r, h) for r, h, _ in regions])
    general = np.zeros(b.n_out, bool)
    for g, (_, _, gen) in enumerate(regions):
        general[int(b.out_off[g]):int(b.out_off[g + 1])] = gen
    return b, general


def make_batch(L, K):
    """The small batch of instance <L, K> -> (batch, mask of the results that belong to the general-path regions)."""
    return _batch_of(instance_regions(L, K))


BIG_REGIONS, BIG_READS = 64, 65   # 4 160 reads >= 4 * NUM_SIMD


def make_big_batch(L, K):
    """4 160 reads of 8 ... 16 rows in 64 regions whose haplotype counts and lengths go round hap_counts / boundary_lengths /
    short_lengths: one class of >= 4 kNumSimd reads -- the EXEC-masked body, one wave per read walking every haplotype group."""
    rng = _rng("big", L, K)
    bl, sl, hc = boundary_lengths(L, K), short_lengths(L, K), hap_counts(L)
    regions = []
    for g in range(BIG_REGIONS):
        root = _rnd(rng, L * K)
        nh = hc[g % len(hc)]
        lens = [bl[g % 3]] + [sl[(g + i) % len(sl)] for i in range(nh - 1)]
        haps = [_hap(rng, root, n) for n in lens]
        reads = [_read(rng, int(n), root, related=(i % 2 == 0)) for i, n in enumerate(rng.integers(8, 17, BIG_READS))]
        regions.append((reads, haps))
    return _to_batch(regions)


def make_run64_batch(L, K):
    """The instance batch and one region of 70 short reads: with force_chain = 64 a full run of CHAIN_MAX_READS and one of six."""
    rng = _rng("run64", L, K)
    root = _rnd(rng, L * K)
    reads = [_read(rng, int(n), root, related=(i % 3 != 2)) for i, n in enumerate(rng.integers(1, 25, 70))]
    haps = [_hap(rng, root, n) for n in (L * K, L * K - 1, K + 1)]
    return _batch_of(instance_regions(L, K) + [(reads, haps, False)])


RUN64_K = {16: 19, 32: 13, 64: 6}   # the instance of each lane count that also runs with runs of 64 reads


def range_ks(lo, hi):
    """K values of a mixed launch of one range: both ends and the middle."""
    return (lo, (lo + hi) // 2, hi)


def make_mixed_batch(L, ks):
    """Regions of several K side by side (region order interleaved): a launch the planner cannot give to a per-K kernel."""
    per_k = [instance_regions(L, K) for K in ks]
    regions = [per_k[i][j] for j in range(len(per_k[0])) for i in range(len(ks))]
    return _batch_of(regions)


ANY_KS = (2, 13, 25)   # the f32 any-K kernel: one launch for every K of a lane count


def region_k(b, L):
    """K per region as the planner picks it under force_L: ceil(longest haplotype / L)."""
    hl = np.diff(b.hap_off.astype(np.int64))
    return [-(-int(hl[int(b.region_hap_off[g]):int(b.region_hap_off[g + 1])].max()) // L) for g in range(b.n_regions)]


# ---- the cases ------------------------------------------------------------------------------------------------------------
FORWARD_CASES = [(L, K) for L in LANES for K in FORWARD_K]
# (L, K, forced streams; 0 = the planner's own choice per region, which at 16 lanes also splits off the remainder items)
CHAIN_CASES = [(L, K, s) for L in CHAIN_LANES for K in CHAIN_K for s in ((0, 1, 2, 4) if L == 16 else (0,))]
RANGE_CASES = [(L, lo, hi) for L in CHAIN_LANES for lo, hi in CHAIN_RANGES]
CHAIN32_CASES = [(L, K, s) for L in CHAIN32_LANES for K in CHAIN32_K for s in ((1, 2, 4) if L == 16 else (1,))]


def forward_id(c):
    return "L%d-K%d" % c


def chain_id(c):
    return "L%d-K%d-%s" % (c[0], c[1], "planner" if c[2] == 0 else "s%d" % c[2])


def range_id(c):
    return "L%d-K%d-%d" % c


def chain_name(name):
    """The plan's name of a chained launch with the per-K kernel's `chain_k<` spelt `chain<` (as the existing tests read it)."""
    return name.replace("chain_k<", "chain<")


def expect_chain_name(name, L, K, streams, f32=False):
    stem = "phmm_forward_chain%s<%d,%d>" % ("_f32" if f32 else "", L, K)
    name = chain_name(name)
    if streams > 1 and L == 16:
        return name == stem + " x%d streams" % streams
    if streams == 1 or L != 16:
        return name == stem
    return name == stem or re.fullmatch(re.escape(stem) + r" x[24] streams", name) is not None


# ---- the GPU side ---------------------------------------------------------------------------------------------------------
_wanted = {}


def _oracle(key, b):
    if key not in _wanted:
        _wanted[key] = oracle.compute_batch(b.as_dict(), n_threads=16)
    return _wanted[key]


@pytest.fixture(scope="module")
def engines():
    from lorikeet_amd import HipPairHMMEngine
    e64, e32 = HipPairHMMEngine(0), HipPairHMMEngine(0, f32_first=True)
    yield e64, e32
    e64.close()
    e32.close()


def _planned(eng, b):
    plan = eng.plan(b)
    name = plan.dominant_kernel
    plan.close()
    return name


def _close_f32(got, want, ctx):
    assert got.shape == want.shape and not np.isnan(got).any() and np.all(got <= 0.0), ctx
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf), ctx
    err = float(np.max(np.abs(got[~inf] - want[~inf])))
    print("%s: max |f32 - oracle| = %.3g" % (ctx, err))
    assert err <= TOL_F32, (ctx, err)


@pytest.mark.gpu
@pytest.mark.parametrize("case", FORWARD_CASES, ids=forward_id)
def test_per_read_instance_equals_the_oracle(engines, case):
    L, K = case
    e64, _ = engines
    small, _ = make_batch(L, K)
    big = make_big_batch(L, K)
    with e64.switches(force_L=L, force_chain=0):
        for what, b in (("small", small), ("big", big)):
            assert _planned(e64, b) == "phmm_forward<%d,%d>" % (L, K), (what, _planned(e64, b))
            _close(e64.compute(b), _oracle((what, L, K), b))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CHAIN_CASES, ids=chain_id)
def test_chained_instance_equals_the_oracle(engines, case):
    L, K, streams = case
    e64, _ = engines
    b, _ = make_batch(L, K)
    with e64.switches(force_L=L, force_chain=RUN, force_streams=streams):
        name = _planned(e64, b)
        assert expect_chain_name(name, L, K, streams), name
        _close(e64.compute(b), _oracle(("small", L, K), b))


@pytest.mark.gpu
@pytest.mark.parametrize("L", CHAIN_LANES)
def test_chained_instance_with_runs_of_64_reads(engines, L):
    e64, _ = engines
    K = RUN64_K[L]
    b, _ = make_run64_batch(L, K)
    with e64.switches(force_L=L, force_chain=CHAIN_MAX_READS, force_streams=1):
        name = _planned(e64, b)
        assert expect_chain_name(name, L, K, 1), name
        _close(e64.compute(b), _oracle(("run64", L, K), b))


@pytest.mark.gpu
@pytest.mark.parametrize("case", RANGE_CASES, ids=range_id)
def test_range_kernel_equals_the_oracle(engines, case):
    L, lo, hi = case
    e64, _ = engines
    b, _ = make_mixed_batch(L, range_ks(lo, hi))
    with e64.switches(force_L=L, force_chain=RUN):
        name = _planned(e64, b)
        # the kernel of the range, not a per-K one: "phmm_forward_chain<L,LO,HI> (K = the dominant class's)"
        assert re.fullmatch(r"phmm_forward_chain<%d,%d,%d> \(K = \d+\)( x[24] streams)?" % (L, lo, hi), name), name
        _close(e64.compute(b), _oracle(("range", L, lo, hi), b))


def _general_reads_are_the_f64_kernels(e64, got, b, general, L, ctx):
    """The runs the f32 kernel leaves alone are redone by the f64 per-read kernel: its results, bit for bit."""
    with e64.switches(force_L=L, force_chain=0):
        per_read = e64.compute(b)
    assert general.any() and np.array_equal(got[general], per_read[general]), ctx


@pytest.mark.gpu
@pytest.mark.parametrize("case", CHAIN32_CASES, ids=chain_id)
def test_chained_f32_instance_equals_the_oracle(engines, case):
    L, K, streams = case
    e64, e32 = engines
    b, general = make_batch(L, K)
    with e32.switches(force_L=L, force_chain=RUN, force_streams=streams):
        name = _planned(e32, b)
        assert expect_chain_name(name, L, K, streams, f32=True), name
        got = e32.compute(b)
    _close_f32(got, _oracle(("small", L, K), b), chain_id(case))
    _general_reads_are_the_f64_kernels(e64, got, b, general, L, chain_id(case))


@pytest.mark.gpu
@pytest.mark.parametrize("L", CHAIN32_LANES)
def test_chained_f32_any_k_kernel_equals_the_oracle(engines, L):
    e64, e32 = engines
    b, general = make_mixed_batch(L, ANY_KS)
    with e32.switches(force_L=L, force_chain=RUN, force_streams=1):
        name = _planned(e32, b)
        assert re.fullmatch(r"phmm_forward_chain_f32_any<%d> \(K = \d+\)" % L, name), name
        got = e32.compute(b)
    _close_f32(got, _oracle(("any", L), b), "any-%d" % L)
    _general_reads_are_the_f64_kernels(e64, got, b, general, L, "any-%d" % L)


# ---- the f32 trust line ---------------------------------------------------------------------------------------------------
TRUST_LINE = -59.0        # log10(likelihood x haplotype length) = log10(2^-196): the kernel's 2^-96 under its 2^100 start
BAND = (-75.0, -45.0)
BAND_CASES = [(90, 16, 1), (90, 16, 2), (90, 16, 4), (90, 32, 1), (300, 16, 1), (300, 16, 2), (300, 16, 4), (300, 32, 1),
              (600, 32, 1)]   # (H, lanes, streams); 600 columns are K = 38 at 16 lanes: beyond the chained kernels (chain_max_k)


def _band_pool(rng, recipe, hap, n_pool):
    """Candidate reads of one recipe.  The share of small terms in the row sums differs between them: "short" has few rows
    with one dominant path, "long" hundreds of paths of nearly equal weight, "block" one good path with a hole."""
    H = len(hap)
    pool = []
    gt = np.frombuffer(b"GT", np.uint8)
    for _ in range(n_pool):
        if recipe == "short":      # high quality, a mismatch in every row: about -4 per row
            n = int(rng.integers(10, 22))
            pool.append((gt[rng.integers(0, 2, n)], rng.integers(24, 46, n), rng.integers(38, 46, n), rng.integers(38, 46, n),
                         rng.integers(36, 46, n)))
        elif recipe == "long":     # low quality, a mismatch in every row: about -0.8 per row
            n = int(rng.integers(50, 95))
            pool.append((gt[rng.integers(0, 2, n)], rng.integers(2, 6, n), rng.integers(38, 46, n), rng.integers(38, 46, n),
                         rng.integers(36, 46, n)))
        else:                      # a window of the haplotype with one block of 10 ... 21 rows that matches nothing
            n = min(int(rng.integers(60, 86)), H)
            s = int(rng.integers(0, H - n + 1))
            bases = hap[s:s + n].copy()
            k = int(rng.integers(10, 22))
            at = int(rng.integers(5, n - k - 5))
            bases[at:at + k] = gt[rng.integers(0, 2, k)]
            pool.append((bases, rng.integers(24, 46, n), rng.integers(38, 46, n), rng.integers(38, 46, n), rng.integers(36, 46, n)))
    return [tuple(np.ascontiguousarray(a, dtype=np.uint8) for a in rd) for rd in pool]


def band_batch(H):
    """For every 0.5-wide step of log10 L + log10 H in BAND the closest reads of three recipes (scored by the oracle against
    the first haplotype), in regions whose other haplotypes are near copies of the first -- and regions with a haplotype
    that holds the read itself, so that one read has pairs on both sides of the line."""
    rng = _rng("band", H)
    ac = np.frombuffer(b"AC", np.uint8)
    first = ac[rng.integers(0, 2, H)]            # no G, no T: the "short" and "long" reads mismatch everywhere
    near = []
    for _ in range(3):
        h = first.copy()
        pos = rng.integers(0, H, 3)
        h[pos] = ac[1 - np.searchsorted(ac, h[pos])]
        near.append(h)
    logH = float(np.log10(H))
    chosen = []
    for recipe in ("short", "long", "block"):
        pool = _band_pool(rng, recipe, first, 900)
        val = oracle.compute_batch(_to_batch([(pool, [first])]).as_dict(), n_threads=16) + logH
        picked = set()
        for target in np.arange(BAND[0], BAND[1] + 0.01, 0.5):
            for i in np.argsort(np.abs(val - target))[:2]:
                picked.add(int(i))
        chosen += [pool[i] for i in sorted(picked)]
    regions = []
    order = rng.permutation(len(chosen))
    for g in range(0, len(order), 13):           # 13 reads a region: runs of 6, 6 and 1
        regions.append(([chosen[i] for i in order[g:g + 13]], [first] + near[:1 + (g // 13) % 3]))
    for g, i in enumerate(order[::7]):           # ... and one haplotype with the read in it
        rd = chosen[i]
        own = first.copy()
        at = int(rng.integers(0, H - len(rd[0]) + 1))
        own[at:at + len(rd[0])] = rd[0]
        regions.append(([rd, chosen[order[(7 * g + 1) % len(order)]], chosen[order[(7 * g + 2) % len(order)]]], [first, own]))
    return _to_batch(regions)


def band_axis(b, want):
    """log10 L + log10 H of every pair (the quantity the kernel's threshold is drawn in)."""
    hl = np.diff(b.hap_off.astype(np.int64))
    x = np.empty_like(want)
    for g in range(b.n_regions):
        nr = int(b.region_read_off[g + 1] - b.region_read_off[g])
        h = hl[int(b.region_hap_off[g]):int(b.region_hap_off[g + 1])]
        x[int(b.out_off[g]):int(b.out_off[g + 1])] = np.tile(np.log10(h), nr)
    return want + x


def band_reads(b, x):
    """Per pair: the smallest and the largest log10 L + log10 H of the pair's READ (the kernel hands over whole reads)."""
    lo, hi = np.empty_like(x), np.empty_like(x)
    for g in range(b.n_regions):
        nr = int(b.region_read_off[g + 1] - b.region_read_off[g])
        nh = int(b.region_hap_off[g + 1] - b.region_hap_off[g])
        m = x[int(b.out_off[g]):int(b.out_off[g + 1])].reshape(nr, nh)
        lo[int(b.out_off[g]):int(b.out_off[g + 1])] = np.repeat(m.min(axis=1), nh)
        hi[int(b.out_off[g]):int(b.out_off[g + 1])] = np.repeat(m.max(axis=1), nh)
    return lo, hi


def band_is_populated(x):
    """At least 100 pairs within 5 of the line on each side, and some within 0.5 on each side."""
    below, above = x[x < TRUST_LINE], x[x >= TRUST_LINE]
    return ((below > TRUST_LINE - 5).sum() >= 100 and (above < TRUST_LINE + 5).sum() >= 100 and
            (below > TRUST_LINE - 0.5).sum() >= 3 and (above < TRUST_LINE + 0.5).sum() >= 3)


@pytest.fixture(scope="module")
def bands():
    out = {}
    for H in sorted({c[0] for c in BAND_CASES}):
        b = band_batch(H)
        want = oracle.compute_batch(b.as_dict(), n_threads=16)
        x = band_axis(b, want)
        assert np.isfinite(want).all() and band_is_populated(x), H
        assert x.max() > -5.0        # the haplotypes that hold their read: a pair far above the line next to one in the band
        out[H] = (b, want, x)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", BAND_CASES, ids=lambda c: "H%d-L%d-s%d" % c)
def test_f32_trust_line(engines, bands, case):
    """Around likelihood x haplotype length = 1e-59 the f32 sweep is at its least accurate, and a threshold drawn too low would
    show here: every pair of the band within TOL_F32 = 1e-5 of the oracle; a read with all its pairs a decade below the line is
    the f64 per-read kernel's result bit for bit (it was handed over), and above the line the results are f32's own (not
    bit-equal to f64: the sweep measures the f32 kernel, not the redo).

    Measured on an MI355X, max |f32 - oracle| against the 1e-5 it is held to (the same for every lane count and stream setting
    of one H -- the f32 cell sequence of a pair does not depend on them):
        H     reads entirely above the line   pairs within 1 above it   reads with a pair below it (handed over: f64)
        90    7.9e-07                         7.2e-07                   2.8e-14
        300   2.9e-06                         1.9e-06                   2.8e-14
        600   4.0e-06                         3.4e-06                   2.8e-14
    The error grows with the number of columns, not towards the line: the argument in the kernel's header holds."""
    H, L, streams = case
    e64, e32 = engines
    b, want, x = bands[H]
    with e32.switches(force_L=L, force_chain=6, force_streams=streams):
        name = _planned(e32, b)
        assert re.match(r"phmm_forward_chain_f32(_any)?<%d[,>]" % L, name), name
        got = e32.compute(b)
    with e64.switches(force_L=L, force_chain=0):
        f64 = e64.compute(b)
    assert not np.isnan(got).any() and np.all(got <= 0.0)
    err = np.abs(got - want)
    lo, hi = band_reads(b, x)
    kept, handed = lo >= TRUST_LINE, lo < TRUST_LINE
    mx = lambda m: float(err[m].max()) if m.any() else 0.0  # noqa: E731
    print("H%d-L%d-s%d: max |f32 - oracle| of reads above the line %.3g (%d pairs), of reads with a pair below it %.3g (%d pairs), of pairs within 1 above it %.3g"
          % (H, L, streams, mx(kept), kept.sum(), mx(handed), handed.sum(), mx(kept & (x < TRUST_LINE + 1))))
    assert float(err.max()) <= TOL_F32
    far_below = hi < TRUST_LINE - 1.0
    assert far_below.sum() >= 100 and np.array_equal(got[far_below], f64[far_below])
    # sensitivity: reads entirely above the line are f32 results -- close to f64, not equal to it
    above = lo > TRUST_LINE + 1.0
    assert above.sum() >= 100 and not np.array_equal(got[above], f64[above])
    assert float(np.max(np.abs(f64 - want))) <= TOL_VS_ORACLE
