"""Test infrastructure: region sets that take phmm_trim_regions past the first pass of compare()'s 256 bytes, past haplotype 63
in the two 64-lane searches for the first failure, and past one region a thread of its scan, built with region_trim_cases.make_hap
and snps.  tests/test_region_trim_wave_table.py (CPU) counts what they cross and checks the witnesses;
tests/test_region_trim_wave_hip.py (GPU) holds the kernels to the restatement.

  late_difference()       a 700-base reference, SNPs at both edges of the active span 1050 .. 1649: the trimmed window is
                          1030 .. 1669, 640 bytes, window byte k is reference index 30 + k.  Triples (the edges alone, one SNP at
                          byte k, another base there) for k = 191, 192, 255, 256, 257, 319, 320, 511, 512, 639; two differences of
                          opposite sign at bytes 70 and 200; differences at 200 and 300; lower against upper case at byte 300
  late_class()            301 haplotypes, those at 3, 70 and 300 equal: none of them the reference, 300 alone, 70 and 300
  late_event_failure()    131 haplotypes, one failing event map at 63, 64, 65 or 130 in each family; two failures of different
                          families at (5, 70) and (64, 130); healthy regions between them
  late_panic()            260 haplotypes, one trim panic at 63, 64, 65 or 200 in each family; two panics of different families at
                          (10, 200) and (64, 200) in both roles; REF_ELIMINATED at 130 behind LENGTH at 129
  many_regions(n)         n = 1025, 2049 regions of 20 reference bases and 2 or 3 haplotypes, every fifth without variation, every
                          eleventh with a duplicate

A set is dict(regions, names, dist, padding) as in tests/region_trim_cases.py; every set here has dist 0 and the default paddings,
so that they also run as one batch.  restated(set name) is computed once per process and not to be changed."""
import functools
import random

import events_restatement as EV
import region_trim_cases as K
import region_trim_restatement as R

LANES = 64
PASS = 256               # compare(): four ballots of 64 bytes
RS = 1000
WINDOW0 = 30             # reference index of window byte 0 in late_difference
LATE_BYTES = (191, 192, 255, 256, 257, 319, 320, 511, 512, 639)
FAIL_AT = (63, 64, 65, 130)
PANIC_AT = (63, 64, 65, 200)
EVENT_FAMILIES = ("ALLELES", "BAD_OPERATOR", "BLOCK", "CIGAR_OVERRUN")
PANIC_FAMILIES = ("LENGTH", "LOCATION", "OPERATOR", "NOT_FOUND")
MANY = (1025, 2049)


def a_set(regions, names):
    assert len(regions) == len(names) == len(set(names))
    return dict(regions=regions, names=names, dist=0, padding=K.DEFAULT)


# ---- compare() behind byte 191 -------------------------------------------------------------------------------------------------------
def late_ref():
    ref = bytearray(K.rand_ref(random.Random(21), 700))
    for k in (70, 200, 300):
        ref[WINDOW0 + k] = ord("G")      # a base with smaller (A, C) and larger (T) ones beside it
    return bytes(ref)


@functools.lru_cache(None)
def late_difference():
    ref = late_ref()
    active, padded, edge = (RS + 50, RS + 649), (RS, RS + 699), [50, 649]
    regions, names = [], []

    def hap(edits, is_ref=False):
        return K.make_hap(ref, RS, sorted(K.snps(ref, edge) + list(edits), key=lambda e: e[1]), is_ref)

    def add(name, haps):
        names.append(name)
        regions.append((ref, RS, active, padded, haps))

    at = lambda k, base: ("S", WINDOW0 + k, base if isinstance(base, int) else ord(base))  # noqa: E731
    for k in LATE_BYTES:
        i = WINDOW0 + k
        add("first_difference_at_%d" % k, [hap([]), hap([at(k, K.other(ref[i]))]), hap([at(k, K.other(ref[i], 2))])])
    # byte 70: A against G; byte 200: G against A -- the earlier one decides
    add("opposite_signs_at_70_and_200", [hap([at(70, "A")]), hap([at(200, "A")])])
    add("opposite_signs_at_70_and_200_reversed", [hap([at(200, "A")]), hap([at(70, "A")])])
    add("differences_at_200_and_300", [hap([at(200, "T")]), hap([at(300, "T")])])
    add("differences_at_200_and_300_reversed", [hap([at(300, "T")]), hap([at(200, "T")])])
    add("lower_case_folds_at_300", [hap([at(300, "C")]), hap([at(300, "c")]), hap([at(300, "T")])])
    add("lower_case_folds_at_300_lower_first", [hap([at(300, "c")]), hap([at(300, "C")])])
    return a_set(regions, names)


# ---- a class whose members lie in different trips -------------------------------------------------------------------------------------
CLASS_AT = (3, 70, 300)
CLASS_REFS = {"no_reference": (), "reference_300": (300,), "references_70_and_300": (70, 300)}


@functools.lru_cache(None)
def late_class():
    ref = K.rand_ref(random.Random(22), 300)
    active, padded, edge = (RS + 100, RS + 199), (RS, RS + 299), [100, 199]     # as order_set: the window is 1080 .. 1219
    regions, names = [], []
    for name, refs in CLASS_REFS.items():
        haps = []
        for i in range(301):
            idx = [180] if i in CLASS_AT else [101 + i % 45, 150 + i // 45]
            haps.append(K.make_hap(ref, RS, K.snps(ref, sorted(edge + idx)), i in refs))
        names.append(name)
        regions.append((ref, RS, active, padded, haps))
    return a_set(regions, names)


# ---- the first failing event map, the first panic -----------------------------------------------------------------------------------
def edge_parts():
    """the reference, the 10-base haplotype and the location of trim_edge_set, its failing and panicking haplotypes by family"""
    ref = K.rand_ref(random.Random(13), 300)
    short = K.cigar_hap([(R.OP_M, 10)], ref)[0]
    wide = (RS, RS + 40)
    event = dict(ALLELES=(short[:4] + short[4:5].lower() + short[5:], [(R.OP_M, 10)], 0, wide, False),
                 BAD_OPERATOR=(short, [(R.OP_M, 5), (R.OP_N, 2), (R.OP_M, 5)], 0, wide, False),
                 BLOCK=(short + b"GG", [(R.OP_M, 5), (R.OP_I, 1), (R.OP_I, 1), (R.OP_M, 5)], 0, wide, False),
                 CIGAR_OVERRUN=(short, [(R.OP_M, 12)], 0, wide, False))
    panic = dict(LENGTH=(short + b"A", [(R.OP_M, 10)], 0, wide, False),
                 LOCATION=(short, [(R.OP_M, 10)], 0, (RS + 3, RS + 12), False),
                 OPERATOR=(b"GG" + short, [(R.OP_S, 2), (R.OP_M, 10)], 0, wide, False),
                 NOT_FOUND=(short[:5], [(R.OP_M, 5)], 0, wide, False),          # the CIGAR ends in front of the stop
                 REF_ELIMINATED=(short[:5] + short[7:], [(R.OP_M, 5), (R.OP_D, 2), (R.OP_M, 3)], 0, wide, True))
    healthy = (short, [(R.OP_M, 10)], 0, wide, False)
    return ref, healthy, event, panic


def edge_region(ref, healthy, n, put, span=(RS + 2, RS + 8)):
    """n haplotypes: the SNP that makes the variation, healthy ones, and put[i] at index i"""
    haps = [K.make_hap(ref, RS, K.snps(ref, [span[0] - RS]))] + [healthy] * (n - 1)
    for i, h in put.items():
        haps[i] = h
    return (ref, RS, span, span, haps)


@functools.lru_cache(None)
def late_event_failure():
    ref, healthy, event, _ = edge_parts()
    regions, names = [], []

    def add(name, put):
        names.append(name)
        regions.append(edge_region(ref, healthy, 131, put))

    for f, fam in enumerate(EVENT_FAMILIES):
        for at in FAIL_AT:
            add("%s_at_%d" % (fam, at), {at: event[fam]})
        add("healthy_behind_%s" % fam, {})
        other = EVENT_FAMILIES[(f + 1) % 4]
        add("%s_at_5_%s_at_70" % (fam, other), {5: event[fam], 70: event[other]})
        add("%s_at_64_%s_at_130" % (fam, other), {64: event[fam], 130: event[other]})
    return a_set(regions, names)


@functools.lru_cache(None)
def late_panic():
    ref, healthy, _, panic = edge_parts()
    regions, names = [], []

    def add(name, put, **kw):
        names.append(name)
        regions.append(edge_region(ref, healthy, 260, put, **kw))

    for f, fam in enumerate(PANIC_FAMILIES):
        for at in PANIC_AT:
            add("%s_at_%d" % (fam, at), {at: panic[fam]})
        add("healthy_behind_%s" % fam, {})
        other = PANIC_FAMILIES[(f + 1) % 4]
        for a, b in ((10, 200), (64, 200)):
            add("%s_at_%d_%s_at_%d" % (fam, a, other, b), {a: panic[fam], b: panic[other]})
            add("%s_at_%d_%s_at_%d" % (other, a, fam, b), {a: panic[other], b: panic[fam]})
    # the span ends inside the reference haplotype's deletion: None for it, which panics -- but LENGTH at 129 comes first
    add("LENGTH_at_129_REF_ELIMINATED_at_130", {129: panic["LENGTH"], 130: panic["REF_ELIMINATED"]}, span=(RS + 2, RS + 6))
    add("REF_ELIMINATED_at_130", {130: panic["REF_ELIMINATED"]}, span=(RS + 2, RS + 6))
    add("REF_ELIMINATED_at_129_LENGTH_at_130", {129: panic["REF_ELIMINATED"], 130: panic["LENGTH"]}, span=(RS + 2, RS + 6))
    return a_set(regions, names)


# ---- more regions than scan threads ------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def many_regions(n):
    rng = random.Random(2300 + n)
    regions, names = [], []
    for g in range(n):
        ref = K.rand_ref(rng, 20)
        rs = 100 + 7 * g
        plain, snp = K.make_hap(ref, rs, (), True), K.make_hap(ref, rs, K.snps(ref, [6 + g % 8]))
        if g % 5 == 4:
            haps = [plain, K.make_hap(ref, rs, ())]                       # no variation: nothing comes out
        elif g % 11 == 0:
            haps = [snp, plain, snp]                                      # a duplicate
        elif g % 3 == 0:
            haps = [plain, snp, K.make_hap(ref, rs, K.snps(ref, [7 + g % 7, 15]))]
        else:
            haps = [plain, snp]
        names.append("region_%d" % g)
        regions.append((ref, rs, (rs + 5, rs + 14), (rs, rs + 19), haps))
    return a_set(regions, names)


SETS = dict(late_difference=late_difference, late_class=late_class, late_event_failure=late_event_failure, late_panic=late_panic,
            many_regions_1025=functools.partial(many_regions, 1025), many_regions_2049=functools.partial(many_regions, 2049))
LATE = ("late_difference", "late_class", "late_event_failure", "late_panic")


@functools.lru_cache(None)
def restated_regions(set_name):
    """R.trim_region of every region of the set"""
    s = SETS[set_name]()
    return [R.trim_region(rg, s["dist"], s["padding"]) for rg in s["regions"]]


def restated(set_name, name):
    return restated_regions(set_name)[SETS[set_name]()["names"].index(name)]


def batch():
    """the four late sets as one call, with many_regions(1025) behind them: (regions, names)"""
    regions, names = [], []
    for s in LATE + ("many_regions_1025",):
        regions += SETS[s]()["regions"]
        names += ["%s-%s" % (s, n) for n in SETS[s]()["names"]]
    return regions, names


# ---- the kernels' loops, restated with a switch each --------------------------------------------------------------------------------
def model_compare(a, b, passes=None, ballots=4):
    """compare(): (length, upper-cased bytes) of a against b, `for (uint32_t c = 0; c < la; c += 256)` with four ballots a pass;
    `passes` and `ballots` cut it short.  (-1 / 0 / 1, the pass that decided, the ballot that decided)"""
    if len(a) != len(b):
        return (-1 if len(a) < len(b) else 1), 0, None
    ua, ub = a.upper(), b.upper()
    n_pass = -(-len(a) // PASS)
    for t in range(n_pass if passes is None else min(passes, n_pass)):
        for q in range(ballots):
            lo = t * PASS + q * LANES
            for k in range(lo, min(lo + LANES, len(a))):
                if ua[k] != ub[k]:
                    return (-1 if ua[k] < ub[k] else 1), t, q
    return 0, max(n_pass - 1, 0), None


def model_first(bad, trips=None):
    """`for (base = 0; base < n && none yet; base += 64)`: the first index that is bad, None without one"""
    hi = len(bad) if trips is None else min(len(bad), trips * LANES)
    for i in range(hi):
        if bad[i]:
            return i
    return None


def model_scan(v, threads=1024, chunk=None):
    """trim_block_scan: (out [n + 1] with None where no thread writes, total)"""
    n = len(v)
    chunk = (n + threads - 1) // threads if chunk is None else chunk
    out, total = [None] * (n + 1), 0
    for t in range(threads):
        lo = min(n, t * chunk)
        for i in range(lo, min(n, lo + chunk)):
            out[i] = total
            total += int(v[i])
    out[n] = total
    return out, total


def event_statuses(region, dist=0):
    """per haplotype the status of its event map"""
    ref, rs, _, _, haps = region
    out = []
    for h in haps:
        try:
            m = EV.event_map(bytes(ref), rs, bytes(h[0]), EV.parse_cigar(h[1]) if isinstance(h[1], str) else list(h[1]), h[2], dist)
            out.append(EV.ALLELES if any(len(vc.alleles) != 2 for vc in m.values()) else 0)      # as build_event_maps
        except EV.Panic as e:
            out.append(e.status)
    return out


def panic_statuses(region, r):
    """per haplotype the panic of its trim to the restated new padded span, 0 without one"""
    out = []
    for h in region[4]:
        hap = (bytes(h[0]), EV.parse_cigar(h[1]) if isinstance(h[1], str) else list(h[1]), h[2], h[3], h[4])
        try:
            t = R.haplotype_trim(hap, r["new_padded"])
            out.append(R.REF_ELIMINATED if isinstance(t, int) and h[4] else 0)
        except R.Panic as e:
            out.append(e.status)
    return out


def windows(region, r):
    """per haplotype its trimmed bases as the set holds them (a duplicate: its representative's), None where none survive"""
    by_source = {src: bases for bases, _, _, _, src in r["out"]}
    out = []
    for i, f in enumerate(r["fates"]):
        out.append(by_source[i] if f >= 0 else by_source[r["dup_of"][i]] if f == R.DUPLICATE else None)
    return out


COUNTS = ("pairs of surviving haplotypes that compare() decides behind its first pass", "of them equal (duplicates)",
          "pairs that ballot q = 3 decides", "regions whose first failing event map is at index >= 64",
          "regions with failing event maps in two trips", "regions whose first trim panic is at index >= 64",
          "regions with trim panics in two trips", "calls of more than 1024 regions", "calls of more than 2048 regions")
EVENT_STATUSES = (EV.BAD_OPERATOR, EV.BLOCK, EV.MERGE, EV.CIGAR_OVERRUN, EV.ALLELES)
TRIM_PANICS = (R.LOCATION, R.LENGTH, R.OPERATOR, R.NOT_FOUND, R.BUILDER, R.REF_ELIMINATED)


def census(regions, restated_list, dist=0):
    """from the regions and R.trim_region of each"""
    c = dict.fromkeys(COUNTS, 0)
    c[COUNTS[7]] += len(regions) > 1024
    c[COUNTS[8]] += len(regions) > 2048
    for region, r in zip(regions, restated_list):
        nh = len(region[4])
        if r["status"] in EVENT_STATUSES and nh > LANES:
            st = event_statuses(region, dist)
            first = model_first([s < 0 for s in st])
            assert st[first] == r["status"]
            c[COUNTS[3]] += first >= LANES
            c[COUNTS[4]] += len({i // LANES for i, s in enumerate(st) if s < 0}) > 1
        if r["status"] in TRIM_PANICS and nh > LANES:
            st = panic_statuses(region, r)
            first = model_first([s < 0 for s in st])
            assert st[first] == r["status"]
            c[COUNTS[5]] += first >= LANES
            c[COUNTS[6]] += len({i // LANES for i, s in enumerate(st) if s < 0}) > 1
        if r["status"] == 0 and r["out"] and max(len(o[0]) for o in r["out"]) > 3 * LANES:
            w = [x for x in windows(region, r) if x is not None and len(x) > 3 * LANES]
            for i, a in enumerate(w):      # (trim_rank_kernel compares every ordered pair: each unordered one counts once here)
                for b in w[:i]:
                    if len(a) != len(b):
                        continue
                    order, t, q = model_compare(a, b)
                    c[COUNTS[0]] += t > 0
                    c[COUNTS[1]] += t > 0 and order == 0
                    c[COUNTS[2]] += q == 3
    return c
