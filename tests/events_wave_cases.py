"""Test infrastructure: regions that take phmm_discover_events past the first trip of its 64-lane loops and its per-locus lists
past 64 entries, built with events_cases.build / region so that bases and CIGAR agree.  tests/test_events_wave_table.py (CPU)
counts what they cross and checks the witnesses; tests/test_events_wave_hip.py (GPU) holds the kernels to the restatement.

  long_elements()             one haplotype per region, 20M <element(s)> 20M at start 2 of a 400-base reference: insertions and
                              deletions of 63 ... 200 bases, the three blocks with a 70-base member, an N at index 63 / 64 of
                              an insertion and as base i == len of a deletion of 63 / 64, each beside its clean twin
  tail_past_64()              an insertion of 70 (64) bases and a deletion of 100 (64) at one anchor: the insertion's merged
                              allele runs from its alt bytes into the reference's tail behind index 64; and two insertions
                              of 70 bases that differ in base 68 alone
  many_alleles()              n = 63, 64, 65, 129, 150 pairwise distinct insertions at one anchor, repeats far behind their
                              originals, a reference-only haplotype last; and one region where two different events give the same
                              merged allele behind 64 others
  many_distinct_haplotypes()  512 and 130 haplotypes whose insertion follows from h
  wide_reference()            4300 reference bases, SNPs around positions 2048 and 4096
  together()                  all of them behind events_cases.multis() in one call

Every set is a list of (name, region); EXPECT[name] is the (reference length, alt length) of the one haplotype's events as
the case was designed, TWIN[name] the clean twin of a case with an N."""
import functools

import numpy as np

import events_cases as K
import events_restatement as R

LANES = 64
EXPECT, TWIN = {}, {}
ANCHOR = 21          # reference index of the last base of the leading 20M at start 2
WIDE_SNPS = (2015, 2016, 2047, 2048, 2049, 2079, 2080, 4063, 4064, 4095, 4096, 4097)
WIDE_START = 1000
MANY = (63, 64, 65, 129, 150)
MAX_HAPS = 512       # PHMM_EVENTS_MAX_HAPS


def bases(seed, n):
    return bytes(np.random.default_rng(seed).choice(list(b"ACGT"), n).astype(np.uint8))


REF400 = bases(400, 400)


def with_base(seq, at, b):
    out = bytearray(seq)
    out[at] = ord(b)
    return bytes(out)


# ---- one haplotype, one long element ------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def long_elements():
    out = []

    def add(name, middle, expect, ref=REF400, lead=("M", 20)):
        out.append((name, K.region(ref, [K.build(ref, [lead] + middle + [("M", 20)], 2)])))
        EXPECT[name] = expect

    for n in (63, 64, 65, 128, 129, 200):
        add("I%d" % n, [("I", bases(1000 + n, n))], [(1, n + 1)])
    for n in (63, 64, 65, 127, 128, 130):
        add("D%d" % n, [("D", n)], [(n + 1, 1)])
    ins = bases(70, 70)
    add("snp_then_I70", [("I", ins)], [(1, 71)], lead=("M", 20, 19))
    add("I70_then_D70", [("I", ins), ("D", 70)], [(71, 71)])
    add("D70_then_I70", [("D", 70), ("I", ins)], [(71, 1), (1, 71)])
    for at in (63, 64):
        add("I70_N_at_%d" % at, [("I", with_base(ins, at, "N"))], [])
        add("I70_clean_at_%d" % at, [("I", with_base(ins, at, "G"))], [(1, 71)])
        TWIN["I70_N_at_%d" % at] = "I70_clean_at_%d" % at
    for n in (63, 64):   # the last deleted base is reference index ANCHOR + n: i == len of the kernel's inclusive loop
        add("D%d_last_base_N" % n, [("D", n)], [], ref=with_base(REF400, ANCHOR + n, "N"))
        TWIN["D%d_last_base_N" % n] = "D%d" % n
    add("D100_N_at_70", [("D", 100)], [], ref=with_base(REF400, ANCHOR + 70, "N"))
    add("D100", [("D", 100)], [(101, 1)])
    TWIN["D100_N_at_70"] = "D100"
    return out


# ---- alt bytes, then the reference's tail ----------------------------------------------------------------------------------------
def tail_region(n_ins, n_del):
    ins = bases(7000 + n_ins, n_ins)
    haps = [K.build(REF400, [("M", 20), ("I", ins), ("M", 60, 30), ("M", 200)], 2), K.build(REF400, [("M", 20), ("D", n_del), ("M", 200)], 2),
            K.build(REF400, [("M", 300)], 2)]
    return K.region(REF400, haps), ins


def late_difference_region():
    """two insertions of 70 bases that differ in their base 68 alone, and the reference: two alleles of 71 bytes"""
    ins = bases(7070, 70)
    other = with_base(ins, 68, "ACGT"["ACGT".index(chr(ins[68])) ^ 1])
    return K.region(REF400, [K.build(REF400, [("M", 20), ("I", i), ("M", 60)], 2) for i in (ins, other)] + [K.build(REF400, [("M", 80)], 2)])


@functools.lru_cache(None)
def tail_past_64():
    return [("I70_beside_D100", tail_region(70, 100)[0]), ("I64_beside_D64", tail_region(64, 64)[0]),
            ("I70_twice_differing_at_68", late_difference_region())]


# ---- more than 64 alleles at one locus -------------------------------------------------------------------------------------------
def many_alleles_region(n):
    """haplotype h carries an insertion of 1 + h bases behind the anchor; for n = 150 every 50th carries the plain G.  Then a
    copy of a haplotype whose event is unique event 64 or later (where n allows), a copy of haplotype 5, the reference."""
    def hap(h):
        ins = b"G" if n == 150 and h % 50 == 0 else bases(9000 + h, 1 + h)
        return K.build(REF400, [("M", 20), ("I", ins), ("M", 40)], 2)
    haps = [hap(h) for h in range(n)]
    haps += [haps[min(70, n - 1)], haps[5], K.build(REF400, [("M", 60)], 2)]
    return K.region(REF400, haps)


HOMO_REF = REF400[:ANCHOR] + b"AGGGGGT" + REF400[ANCHOR + 7:]


def equal_alleles_region():
    """70 distinct insertions at an anchor A before GGGGG, then AG -> A, then the block of an insertion GG with the deletion of
    GGG: under the merged reference AGGG both are AGG, two different events and one allele, whose first copy is alt 70."""
    def hap(middle):
        return K.build(HOMO_REF, [("M", 20)] + middle + [("M", 40)], 2)
    haps = [hap([("I", b"C" + bytes(b"ACGT"[(h >> (2 * d)) & 3] for d in range(4)))]) for h in range(70)]
    haps += [hap([("D", 1)]), hap([("I", b"GG"), ("D", 3)]), hap([])]
    return K.region(HOMO_REF, haps)


@functools.lru_cache(None)
def many_alleles():
    return [("%d_insertions" % n, many_alleles_region(n)) for n in MANY] + [("equal_alleles_behind_70", equal_alleles_region())]


# ---- every haplotype another one --------------------------------------------------------------------------------------------------
def distinct_region(n_haps):
    haps = []
    for h in range(n_haps):
        k = (h // 3) % 160   # 160 insertions per anchor: from haplotype 480 on they repeat
        ins = bytes(b"ACGT"[(k >> (2 * d)) & 3] for d in range(4)) + b"T" * (k % 3)
        haps.append(K.build(REF400, [("M", 10 + h % 3), ("I", ins), ("M", 50, 5 + h % 40)], 2))
    return K.region(REF400, haps)


@functools.lru_cache(None)
def many_distinct_haplotypes():
    return [("512_haplotypes", distinct_region(MAX_HAPS)), ("130_haplotypes", distinct_region(130))]


# ---- a reference above 2048 and 4096 bases -----------------------------------------------------------------------------------------
@functools.lru_cache(None)
def wide_reference():
    ref = bases(4300, 4300)
    haps = [K.build(ref, [("M", 4290) + WIDE_SNPS], 0), K.build(ref, [("M", 4290) + WIDE_SNPS[::2]], 0)]
    whole = K.region(ref, haps, ref_start=WIDE_START, window=(WIDE_START, WIDE_START + 4299))
    cut = K.region(ref, haps, ref_start=WIDE_START, window=(WIDE_START + 2048, WIDE_START + 4095))
    return [("whole_window", whole), ("window_2048_4095", cut)]


SETS = dict(long_elements=long_elements, tail_past_64=tail_past_64, many_alleles=many_alleles,
            many_distinct_haplotypes=many_distinct_haplotypes, wide_reference=wide_reference)


def named(set_name, name):
    return dict(SETS[set_name]())[name]


def new_regions():
    return [rg for s in SETS.values() for _, rg in s()]


def together():
    """(regions, index of the first new one): events_cases.multis() in front, then every set"""
    front = [rg for _, rg, _ in K.multis()]
    return front + new_regions(), len(front)


@functools.lru_cache(None)
def _restated(set_name, dist, include_spanning):
    return [R.discover([rg], dist, include_spanning) for _, rg in SETS[set_name]()]


def restated(set_name, name, dist=0, include_spanning=True):
    """R.discover of one region alone, computed once per process and not to be changed"""
    return _restated(set_name, dist, include_spanning)[[n for n, _ in SETS[set_name]()].index(name)]


# ---- the census --------------------------------------------------------------------------------------------------------------------
COUNTS = ("insertions of >= 64 bases that yield an event", "deletions of >= 64 bases that yield an event",
          "insertions with a base that is not regular at index >= 64", "deletions with a base that is not regular at index >= 64",
          "loci with more than 64 alleles", "loci with more than 128 alleles", "dedup hits on unique event >= 64",
          "haplotypes >= 64 on alt index >= 64", "alleles of exactly 64 bytes", "alleles of exactly 65 bytes", "alleles of more than 65 bytes",
          "alleles that go from alt to reference tail at index >= 64", "loci at reference position >= 2048", "loci at reference position >= 4096")
ALLELE_BYTES = COUNTS[8:11]   # events_cases' M65_dense and M129_dense at distance 3 are one MNP each: not new here


def walk(rg):
    """(haplotype, operator, length, event start, the bases the kernel's loop tests from index 0) of every I and D element that
    can propose an event, as process_cigar_for_initial_events walks them; stops where it would panic."""
    ref = rg["ref"]
    for h, (hap, cigar, hs) in enumerate(rg["haps"]):
        ref_pos, ap = hs, 0
        for ci, (op, ln) in enumerate(cigar):
            if op == R.OP_I:
                if ref_pos > 0 and ref_pos - 1 < len(ref) and 0 < ci < len(cigar) - 1 and ap + ln <= len(hap):
                    yield h, "I", ln, rg["ref_start"] + ref_pos - 1, hap[ap:ap + ln]
                ap += ln
            elif op == R.OP_S:
                ap += ln
            elif op == R.OP_D:
                if ref_pos > 0 and ref_pos + ln <= len(ref):
                    yield h, "D", ln, rg["ref_start"] + ref_pos - 1, ref[ref_pos - 1:ref_pos + ln]
                ref_pos += ln
            elif op in (R.OP_M, R.OP_EQ, R.OP_X):
                ref_pos += ln
                ap += ln
            else:
                break


def census(regions, dist=0, include_spanning=True, margin=2):
    c = dict.fromkeys(COUNTS, 0)
    for rg in regions:
        r = R.discover_region(rg["ref"], rg["ref_start"], rg["haps"], rg["window"], rg["contig_length"], dist, include_spanning, margin)
        for h, op, ln, start, tested in walk(rg):
            vc = r["maps"][h].get(start) if r["maps"] else None
            if ln >= LANES and vc is not None and (len(vc.alt) >= ln + 1 if op == "I" else len(vc.ref) >= ln + 1):
                c[COUNTS[0 if op == "I" else 1]] += 1
            if any(b not in R.REGULAR for b in tested[LANES:]):
                c[COUNTS[2 if op == "I" else 3]] += 1
        for ev in r["events"]:
            n, loc = len(ev["alleles"]), ev["loc"]
            c[COUNTS[4]] += n > 64
            c[COUNTS[5]] += n > 128
            unique = []   # get_variant_contexts_from_active_haplotypes: the first occurrence by (start, alleles)
            for m in r["maps"]:
                for vc in R.get_overlapping_events(m, loc):
                    if include_spanning or vc.start == loc:
                        if vc.key in unique:
                            c[COUNTS[6]] += unique.index(vc.key) >= LANES
                        else:
                            unique.append(vc.key)
            c[COUNTS[7]] += sum(h >= LANES and a - 1 >= LANES for h, a in enumerate(ev["hap_allele"]))
            for a in ev["alleles"]:
                c[COUNTS[8]] += len(a) == 64
                c[COUNTS[9]] += len(a) == 65
                c[COUNTS[10]] += len(a) > 65
            for start, alleles in unique:
                c[COUNTS[11]] += start == loc and len(alleles[0]) < len(ev["alleles"][0]) and len(alleles[1]) >= LANES
            c[COUNTS[12]] += loc - rg["ref_start"] >= 2048
            c[COUNTS[13]] += loc - rg["ref_start"] >= 4096
    return c
