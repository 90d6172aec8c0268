"""Test infrastructure: calls that take phmm_assembly_regions past the first trip of its 64-lane loops, past one entry a thread
of its 1024-thread scans and past 2^32 in its positions, built with assembly_regions_cases.make / profile / read / runs.
tests/test_assembly_regions_wave_table.py (CPU) counts what they cross and checks the witnesses;
tests/test_assembly_regions_wave_hip.py (GPU) holds the kernels to the restatement.

  scan_profiles_N        N = 1023, 1024, 1025, 2049 profiles of 0 .. 12 equal states, every seventh empty; max_region_size 4 and
                         propagation 0, so a profile gives 0 .. 3 regions
  scan_pairs_N           N (region, sample) pairs: two profiles of inactive states in two windows, max_region_size 3, each
                         profile's last region of 2 states.  1023 = 341 x 3, 1026 = 342 x 3 and 2049 = 683 x 3; 1024 and 1025
                         have no factor 3 and are 512 x 2 and 205 x 5.  Seeded reads: pair_count takes
                         four values and more, is above 0 for most pairs and 0 for at least one in twenty
  span_dense_N_firstF    F = 0, 1, 63 inactive states, N = 4096, 4097, 4160, 8193 active ones of which about half are above 0.05,
                         20 inactive; max_region_size N + 10: one region.  At the threshold 0.002 a state outside an active run
                         cannot be above 0.05, so the dense plane holds no bit beside this region ...
  span_sparse_N_firstF   ... and this is its mirror at the threshold 0.5: F active states, N inactive ones seeded over (0.01, 0.5),
                         20 active.  Here the words at both ends of the region hold set bits of its neighbours
  cut_*                  max_region_size 4100 (word 64, bit 4): runs that end around it, from list index 0 and from 37; the cut
                         site among 4095 and 4099 candidates; a forced tail that ends in word 65
  cigar_N_elements       N = 63, 64, 65, 130 CIGAR elements of every operator: the read reaches the padded span through its last
                         element alone, its twin without that element does not; reads of 64 .. 300 bases with seeded qualities
  members_N              N = 63, 64, 65, 128, 129 overlapping reads among 200 candidates of one (region, sample), a second sample
                         with another count
  positions_past_2_32    a profile whose regions straddle 2^32, one that ends at position 2^62 - 1 on a contig of 2^62 - 1
  together               read_cases()["two_windows"] in front of parts built like the above, under its parameters, in one call

CASES maps a name to the builder of (arrays, parameters); case(name) builds it once per process, restated(name) restates it once
per process.  Neither result is to be changed."""
import functools

import numpy as np

import assembly_regions_cases as K
import assembly_regions_restatement as R

LANES = 64
SCAN_THREADS = 1024      # REG_SCAN_THREADS
MAX_4100 = 4100          # word 64, bit 4
M, I, D, N, S, H, P, EQ, X = range(9)
SCAN_SIZES = (1023, 1024, 1025, 2049)
PAIR_SHAPES = {1023: (341, 3), 1024: (512, 2), 1025: (205, 5), 1026: (342, 3), 2049: (683, 3)}
SPAN_SIZES, SPAN_FIRST = (4096, 4097, 4160, 8193), (0, 1, 63)
CIGAR_SIZES = (63, 64, 65, 130)
MEMBER_SIZES = (63, 64, 65, 128, 129)
QUAL_LENGTHS = (64, 65, 128, 129, 300)
CASES = {}


def f32(x):
    return float(np.float32(x))


# ---- the scans --------------------------------------------------------------------------------------------------------------------
def scan_profiles(n):
    rng = np.random.default_rng(1000 + n)
    ps = []
    for k in range(n):
        length = 0 if k % 7 == 3 else int(rng.integers(0, 13))
        ps.append(K.profile(K.runs((1.0 if k % 2 else 0.0, length)), start=int(rng.integers(0, 5000)), contig=1 << 20))
    return K.make(ps, max_region_size=4, max_prob_propagation=0, min_region_size=1, extension=3)


def pair_parts(n_regions, n_samples, seed, max_region_size=3, per_state=0.2, start=1000):
    """(profiles, groups): two profiles of inactive states in windows 0 and 1 that give n_regions regions of max_region_size
    states, each profile's last of one less; per sample and window seeded short reads over the profile's span"""
    rng = np.random.default_rng(seed)
    first = n_regions // 2
    ps, groups = [], []
    for w, regions in enumerate((first, n_regions - first)):
        states = regions * max_region_size - 1
        ps.append(K.profile(K.runs((0.0, states)), start=start + 5000 * w, contig=1 << 28, window=w))
        for s in range(n_samples):
            pos = sorted(int(x) for x in rng.integers(start + 5000 * w - 5, start + 5000 * w + states, int(states * per_state * (1 + s % 2))))
            groups.append([K.read(p, [(M, int(rng.integers(1, 7)))]) for p in pos])
    return ps, groups


def scan_pairs(n):
    regions, samples = PAIR_SHAPES[n]
    ps, groups = pair_parts(regions, samples, 2000 + n)
    return K.make(ps, groups, n_samples=samples, max_region_size=3, max_prob_propagation=0, extension=1)


# ---- the density ------------------------------------------------------------------------------------------------------------------
def span_case(n, first, sparse):
    """dense: `first` inactive states, n active ones, 20 inactive, threshold 0.002; sparse: the mirror at threshold 0.5"""
    rng = np.random.default_rng(3000 + n + first + (7 if sparse else 0))
    if sparse:
        inside = [f32(rng.uniform(0.01, 0.05)) if rng.random() < 0.5 else f32(rng.uniform(0.06, 0.5)) for _ in range(n)]
        out = lambda k: [f32(rng.uniform(0.6, 1.0)) for _ in range(k)]  # noqa: E731
    else:
        inside = [f32(rng.uniform(0.01, 0.05)) if rng.random() < 0.5 else f32(rng.uniform(0.06, 1.0)) for _ in range(n)]
        out = lambda k: [f32(rng.uniform(0.0, 0.002)) for _ in range(k)]  # noqa: E731
    inside[-2:] = [f32(0.02), f32(0.4)]       # the region's last state is above 0.05 whatever the seed, the one before it is not
    probs = out(first) + inside + out(20)
    return K.make([K.profile(probs, start=500)], max_region_size=n + 10, max_prob_propagation=0, min_region_size=1, extension=5,
                  threshold=0.5 if sparse else K.THRESHOLD)


# ---- the boundary and the cut site behind 64 words -------------------------------------------------------------------------------
def cut_case(probs, mn=5, **kw):
    return K.make([K.profile(probs, start=100)], min_region_size=mn, max_region_size=MAX_4100, max_prob_propagation=0, extension=10, **kw)


@functools.lru_cache(None)
def cut_cases():
    c = {}
    for lead in (0, 37):   # the run from list index 0, and from 37 behind a region of the other kind
        for n in (4100, 4101, 4102, 4300):      # inactive: not found over 65 words, e = limit; 4101 and 4102 end inside word 64 behind bit 4
            c["cut_inactive_%d_lead%d" % (n, lead)] = cut_case(K.runs((1.0, lead), (0.0, n), (1.0, 80)))
        for n in (4099, 4100, 4102):            # active: 4102 is cut at 4100, where the mask of the last word ends the search
            c["cut_active_%d_lead%d" % (n, lead)] = cut_case(K.runs((0.0, lead), (1.0, n), (0.0, 80)))
    base = K.runs((1.0, 4200), (0.0, 80))

    def site(name, edits, mn=5, lead=0):
        p = list(base)
        for i, v in edits.items():
            p[i] = v
        c["cut_site_" + name] = cut_case(K.runs((0.0, lead)) + p, mn=mn)

    site("one_minimum_4090", {4090: 0.5})
    site("one_minimum_70", {70: 0.5})
    site("one_minimum_70_lead37", {70: 0.5}, lead=37)
    site("equal_100_and_4000", {100: 0.5, 4000: 0.5})
    site("equal_64_apart", {10: 0.5, 74: 0.5})
    site("equal_4096_apart", {2: 0.5, 4098: 0.5}, mn=1)        # 4099 candidates from index 1
    site("lower_early_beats_equal_late", {9: 0.25, 100: 0.5, 4000: 0.5})
    site("none", {})
    site("none_min_size_1", {}, mn=1)
    site("nan_4000_beside_200", {200: 0.5, 4000: K.NAN})       # a NaN is inactive: the boundary, in word 62
    site("nan_4097_beside_200", {200: 0.5, 4097: K.NAN})       # ... and in word 64: found in the second trip, no cut site
    site("nan_behind_end", {200: 0.75, 4099: 0.5, 4100: K.NAN})  # 4099 <= NaN is false: no minimum, 200 wins
    site("minimum_at_end_minus_1", {4099: 0.5})
    site("minimum_at_end", {4100: 0.5})
    # the forced short tail: 100 inactive states, then 4090 active ones that end the list in word 65 (rem < max)
    c["cut_forced_tail_word65"] = cut_case(K.runs((0.0, 100), (1.0, 4090)))
    return c


# ---- reads ------------------------------------------------------------------------------------------------------------------------
FLAT50 = dict(max_region_size=50, max_prob_propagation=0, extension=10)   # one region 1000 .. 1049, padded 990 .. 1059
OPS = (M, I, D, N, S, EQ, X, H, P)


def long_cigar(n):
    """n elements over every operator with lengths 1 .. 3, the last one 2M"""
    return [(OPS[(i * 5) % 9], 1 + i % 3) for i in range(n - 1)] + [(M, 2)]


def quals_for(rng, cigar):
    n = sum(ln for op, ln in cigar if op in (M, I, S, EQ, X))
    q = rng.integers(0, 94, n)
    q[rng.random(n) < 0.1] = 255
    return [int(x) for x in q]


def ref_len(cigar):
    return sum(ln for op, ln in cigar if op in (M, D, N, EQ, X))


def cigar_reads(n, rng, padded_start=990):
    """the read of n elements that ends one base inside the padded span, its twin without the last element, which ends in front
    of it, for n > 64 the twin of 64 elements; then reads of QUAL_LENGTHS bases inside the region"""
    full = long_cigar(n)
    pos = padded_start - ref_len(full[:-1])      # the twin's end (exclusive) is the padded start: not fetched
    reads = [K.read(pos, full, quals_for(rng, full)), K.read(pos, full[:-1], quals_for(rng, full[:-1]))]
    if n > LANES:
        reads.append(K.read(pos, full[:LANES], quals_for(rng, full[:LANES])))
    for k, length in enumerate(QUAL_LENGTHS):
        c = [(M, length)]
        reads.append(K.read(padded_start + 10 + k, c, quals_for(rng, c)))
    return reads


def cigar_case(n):
    rng = np.random.default_rng(4000 + n)
    return K.make([K.profile(K.runs((1.0, 50)), start=1000, contig=5000)], [cigar_reads(n, rng)], **FLAT50)


def member_reads(n, rng, candidates=200, padded_start=990):
    """a long read at 700 that reaches the region, then candidates - 1 reads at 710, 711, ...: n - 1 of them reach the padded
    span, the others end in front of it"""
    reach = set(int(x) for x in rng.choice(candidates - 1, n - 1, replace=False))
    reads = [K.read(700, [(M, 10), (N, 300), (M, 10)])]
    for i in range(candidates - 1):
        reads.append(K.read(710 + i, [(M, padded_start - 700 + int(rng.integers(0, 60)))] if i in reach else [(M, int(rng.integers(1, 6)))]))
    return reads


def members_case(n):
    rng = np.random.default_rng(5000 + n)
    groups = [member_reads(n, rng), member_reads(n // 2 + 3, rng, candidates=150)]
    return K.make([K.profile(K.runs((1.0, 50)), start=1000, contig=5000)], groups, n_samples=2, **FLAT50)


# ---- positions --------------------------------------------------------------------------------------------------------------------
P32, P62 = 1 << 32, 1 << 62


def position_parts(n_samples, rng):
    """(profiles, groups): 700 states from 2^32 - 20 on a contig of 2^33 in window 0; 10 000 states from 2^62 - 10 000, the last
    at the contig's length 2^62 - 1, in window 1"""
    ps = [K.profile(K.random_probs(rng, 700), start=P32 - 20, contig=1 << 33, window=0),
          K.profile(K.random_probs(rng, 10000), start=P62 - 10000, contig=P62 - 1, window=1)]
    groups = []
    for w, (lo, hi) in enumerate(((P32 - 120, P32 + 700), (P62 - 600, P62 - 1))):
        for s in range(n_samples):
            pos = sorted(lo + int(x) for x in rng.integers(0, hi - lo, 60 + 30 * s))
            groups.append([K.read(p, [(M, int(rng.integers(1, 90)))]) for p in pos])
    return ps, groups


def positions_case():
    ps, groups = position_parts(2, np.random.default_rng(6000))
    return K.make(ps, groups, n_samples=2, max_region_size=300, min_region_size=20, max_prob_propagation=0, extension=40)


# ---- several in one call ----------------------------------------------------------------------------------------------------------
def join(parts):
    """the arrays of several calls with reads and one sample count as one call: lists, windows and reads one behind the other"""
    out = dict(parts[0])
    for a in parts[1:]:
        assert a["n_samples"] == out["n_samples"]
        shift = dict(profile_first=len(out["profile_prob"]), profile_window=out["n_windows"], group_read_off=len(out["read_pos"]),
                     read_cigar_off=len(out["read_cigar"]), read_off=len(out["read_quals"]))
        for k in ("profile_prob", "profile_len", "profile_start", "profile_stop", "profile_contig_length", "read_pos", "read_cigar", "read_quals"):
            out[k] = np.concatenate([out[k], a[k]])
        for k in ("profile_first", "profile_window"):
            out[k] = np.concatenate([out[k], a[k] + np.uint32(shift[k])])
        for k in ("group_read_off", "read_cigar_off", "read_off"):
            out[k] = np.concatenate([out[k], a[k][1:] + np.uint32(shift[k])])
        out["n_windows"] += a["n_windows"]
    return out


@functools.lru_cache(None)
def together_parts():
    """[(name, arrays)], parameters: two_windows and parts with two samples under two_windows' parameters (max_region_size 40,
    propagation 0, extension 15).  The pairs part alone gives 526 x 2 pairs, so the call's scan over pairs has n > 1024."""
    first, p = K.read_cases()["two_windows"]
    rng = np.random.default_rng(7000)
    flat = [K.profile(K.runs((1.0, 50)), start=1000, contig=5000)]
    parts = [("two_windows", first),
             ("members", K.make(flat, [member_reads(129, rng), member_reads(65, rng, candidates=150)], n_samples=2)[0]),
             ("cigar", K.make(flat, [cigar_reads(130, rng, padded_start=985), cigar_reads(65, rng, padded_start=985)], n_samples=2)[0]),
             ("positions", K.make(*position_parts(2, rng), n_samples=2)[0]),
             ("pairs", K.make(*pair_parts(526, 2, 7001, max_region_size=40, per_state=0.02), n_samples=2)[0])]
    return parts, p


def together():
    parts, p = together_parts()
    return join([a for _, a in parts]), p


for _n in SCAN_SIZES:
    CASES["scan_profiles_%d" % _n] = functools.partial(scan_profiles, _n)
for _n in sorted(PAIR_SHAPES):
    CASES["scan_pairs_%d" % _n] = functools.partial(scan_pairs, _n)
for _n in SPAN_SIZES:
    for _f in SPAN_FIRST:
        CASES["span_dense_%d_first%d" % (_n, _f)] = functools.partial(span_case, _n, _f, False)
        CASES["span_sparse_%d_first%d" % (_n, _f)] = functools.partial(span_case, _n, _f, True)
for _name in cut_cases():
    CASES[_name] = functools.partial(lambda name: cut_cases()[name], _name)
for _n in CIGAR_SIZES:
    CASES["cigar_%d_elements" % _n] = functools.partial(cigar_case, _n)
for _n in MEMBER_SIZES:
    CASES["members_%d" % _n] = functools.partial(members_case, _n)
CASES["positions_past_2_32"] = positions_case
CASES["together"] = together


@functools.lru_cache(None)
def case(name):
    return CASES[name]()


def restate(a, p, **kw):
    return R.assembly_regions(a, p["extension"], p["min_region_size"], p["max_region_size"], p["max_prob_propagation"],
                              np.float32(p["threshold"]), p["max_input_depth"], **kw)


@functools.lru_cache(None)
def restated(name):
    return restate(*case(name))


# ---- the kernels' loops, restated with a switch each --------------------------------------------------------------------------------
# What a loop gives when it stops after its first trip (`trips=1`), when a scan thread takes one entry whatever n (`per=1`),
# when the mask of the last word is left out (`mask=False`), when positions keep 32 bits (`bits=32`).  With the switches as
# they are the models give the restated result, which the table test asserts for every case.
def planes(a, p, k):
    """the states of profile k as booleans: active, dense"""
    f, n = int(a["profile_first"][k]), int(a["profile_len"][k])
    q = np.asarray(a["profile_prob"][f:f + n], np.float32)
    with np.errstate(invalid="ignore"):
        return q > np.float32(p["threshold"]), q > R.DENSITY_TOLERANCE, q


def words(first, n):
    return first >> 6, (first + n - 1) >> 6


def model_boundary(active, cur, limit, trips=None, mask=True):
    """regions_cut_kernel: for (uint32_t base = w0; base <= w1; base += 64) -- the first state in [cur, cur + limit) that differs
    from state cur, as an offset; limit when none does.  (index, second-or-later trips taken)"""
    w0, w1 = words(cur, limit)
    n = len(active)
    is_active = bool(active[cur])
    later = 0
    for t, base in enumerate(range(w0, w1 + 1, LANES)):
        if trips is not None and t >= trips:
            break
        later += t > 0
        lo, hi = max(base * 64, cur), min((base + LANES) * 64, (w1 + 1) * 64)
        if mask:
            hi = min(hi, cur + limit)
        for i in range(lo, hi):     # (a bit behind the list is 0: it differs from an active run)
            if (bool(active[i]) if i < n else False) != is_active:
                return i - cur, later
    return limit, later


def is_min(q, s):
    """the minimum plane: p[s] <= p[s + 1] && p[s] < p[s - 1] for 1 <= s < len - 1"""
    return 1 <= s < len(q) - 1 and bool(q[s] <= q[s + 1]) and bool(q[s] < q[s - 1])


def model_cut_site(q, cur, e, min_size, trips=None):
    """for (uint32_t i = p.min_size + lane; i < e; i += 64): the smallest minimum, the highest index among equals, as e"""
    hi = e if trips is None else min(e, min_size + trips * LANES)
    best, best_i = None, None
    for i in range(min_size, hi):
        v = q[cur + i]
        if i >= 1 and is_min(q, cur + i) and bool(v < R.F32_MAX) and (best is None or bool(v <= best)):
            best, best_i = v, i
    return e if best is None else best_i + 1


def model_density(dense, first, n, size, trips=None, mask=True):
    """regions_span_kernel: for (uint32_t w = w0 + lane; w <= w1; w += 64), both masks, one division"""
    w0, w1 = words(first, n)
    last = w1 if trips is None else min(w1, w0 + trips * LANES - 1)
    hi = (last + 1) * 64 if (last < w1 or not mask) else first + n     # mask: that of the region's last word
    c = int(np.count_nonzero(dense[first:min(hi, len(dense))]))
    return np.float32(c) / np.float32(size)


def model_scan(v, per=None):
    """regions_block_scan: (off [n + 1] with None where no thread writes, total)"""
    n = len(v)
    per = (n + SCAN_THREADS - 1) // SCAN_THREADS if per is None else per
    off, total = [None] * (n + 1), 0
    for t in range(SCAN_THREADS):
        b, e = min(t * per, n), min(min(t * per, n) + per, n)
        for i in range(b, e):
            off[i] = total
            total += int(v[i])
    off[n] = total
    return off, total


def model_reflen(cigar, trips=None):
    """regions_read_kernel: for (uint32_t c = p.cigar_off[r] + lane; c < p.cigar_off[r + 1]; c += 64)"""
    return R.reference_length(cigar if trips is None else cigar[:trips * LANES])


def model_qsum(quals, trips=None):
    return sum(int(x) for x in (quals if trips is None else quals[:trips * LANES]))


def candidates(a, ends, g, ps, pe, bits=64):
    """regions_count_kernel's two binary searches: reads [lo, hi) of group g"""
    m = (1 << bits) - 1
    r0, r1 = int(a["group_read_off"][g]), int(a["group_read_off"][g + 1])
    hi = r0
    while hi < r1 and (int(a["read_pos"][hi]) & m) <= pe:
        hi += 1
    lo, run = r0, None
    while lo < hi:
        run = ends[lo] if run is None else max(run, ends[lo])
        if run > ps:
            break
        lo += 1
    return lo, hi


def model_members(a, ends, g, ps, pe, trips=None, bits=64):
    """regions_members_kernel: for (uint32_t base = lo; base < hi; base += 64)"""
    lo, hi = candidates(a, ends, g, ps, pe, bits)
    if trips is not None:
        hi = min(hi, lo + trips * LANES)
    return [i for i in range(lo, hi) if ends[i] > ps]


def read_ends(a, trips=None, bits=64):
    m = (1 << bits) - 1
    out = []
    for r in range(len(a["read_pos"])):
        n = model_reflen(a["read_cigar"][a["read_cigar_off"][r]:a["read_cigar_off"][r + 1]], trips)
        out.append(((int(a["read_pos"][r]) & m) + max(n, 1)) & m)
    return out


COUNTS = ("scans over profiles with n > 1024", "scans over pairs with n > 1024", "scans with n > 2048 (per = 3)",
          "regions of more than 64 words (the popcount's second trip)", "of them with states above 0.05",
          "boundary searches that take a second trip", "of them in an active run", "of them from a list index that is no multiple of 64",
          "of them that find nothing", "of them where the last word's mask hides a differing state",
          "cut-site searches in a run of more than 64 words", "cut-site searches over more than 4096 candidates",
          "reads of more than 64 CIGAR elements", "reads of more than 128 CIGAR elements", "pairs of more than 64 members",
          "pairs of more than 128 members", "positions at or above 2^32")
# what assembly_regions_cases.all_cases() already reaches: boundary_word70's search from index 0 for the first active state finds it
# in its second trip, that region of 4485 states has no state above 0.05, and two_windows has one pair of 72 members
ALREADY = {COUNTS[3]: 1, COUNTS[5]: 1, COUNTS[14]: 1}


def regions_of(a, want):
    """(profile, list index of the first state, states, flags) per region"""
    off = [int(x) for x in want["profile_region_off"]]
    for k in range(len(off) - 1):
        for r in range(off[k], off[k + 1]):
            yield r, k, int(want["region_start"][r]) - int(a["profile_start"][k]), int(want["region_states"][r]), int(want["region_flags"][r])


def census(a, p, want):
    c = dict.fromkeys(COUNTS, 0)
    n_profiles, n_regions = len(a["profile_len"]), int(want["required"][0])
    reads = a.get("group_read_off") is not None
    n_pairs = n_regions * int(a["n_samples"]) if reads else 0
    c[COUNTS[0]] += n_profiles > SCAN_THREADS
    c[COUNTS[1]] += n_pairs > SCAN_THREADS
    c[COUNTS[2]] += (n_profiles > 2 * SCAN_THREADS) + (n_pairs > 2 * SCAN_THREADS)
    kept = {}
    for r, k, cur, e, flags in regions_of(a, want):
        if k not in kept:
            kept[k] = planes(a, p, k)
        active, dense, q = kept[k]
        w0, w1 = words(cur, e)
        if w1 - w0 >= LANES:
            c[COUNTS[3]] += 1
            c[COUNTS[4]] += bool(np.count_nonzero(dense[cur:cur + e]))
        limit = min(len(active) - cur, p["max_region_size"])
        found, later = model_boundary(active, cur, limit)
        if later:
            c[COUNTS[5]] += 1
            c[COUNTS[6]] += bool(active[cur])
            c[COUNTS[7]] += cur % 64 != 0
            c[COUNTS[8]] += found == limit
            c[COUNTS[9]] += model_boundary(active, cur, limit, mask=False)[0] != found
        if bool(active[cur]) and found == p["max_region_size"] and found >= p["min_region_size"]:
            c[COUNTS[10]] += found > LANES * 64
            c[COUNTS[11]] += found - p["min_region_size"] > 4096
    if reads:
        n_cigar = np.diff(np.asarray(a["read_cigar_off"], np.int64)) if len(a["read_pos"]) else np.zeros(0, np.int64)
        c[COUNTS[12]] += int(np.count_nonzero(n_cigar > LANES))
        c[COUNTS[13]] += int(np.count_nonzero(n_cigar > 2 * LANES))
        per_pair = np.diff(np.asarray(want["region_read_off"], np.int64))
        c[COUNTS[14]] += int(np.count_nonzero(per_pair > LANES))
        c[COUNTS[15]] += int(np.count_nonzero(per_pair > 2 * LANES))
        c[COUNTS[16]] += int(np.count_nonzero(np.asarray(a["read_pos"], np.int64) >= P32))
    for k in ("region_start", "region_end", "region_padded_start", "region_padded_end"):
        c[COUNTS[16]] += sum(int(x) >= P32 for x in want[k])
    return c
