"""Test infrastructure: the regions tests/test_region_trim_hip.py runs phmm_trim_regions on, and whose reach
tests/test_region_trim_oracle.py counts on the CPU.  A region is what lorikeet_amd.trim.Region lists: (ref, ref_start, active,
padded, haps) with haps as (bases, cigar, hap_start, (loc start, loc end), is_ref).  A set is dict(regions, dist, padding)."""
import itertools
import random

import region_trim_restatement as R

SMALL = (5, 12, 12, 25)       # paddings that stay inside the test regions
DEFAULT = (20, 75, 75, 25)
BASES = b"ACGT"


def rand_ref(rng, n):
    return bytes(rng.choice(BASES) for _ in range(n))


def other(b, k=1):
    """an upper-case base that differs from b"""
    return BASES[(BASES.index(bytes([b]).upper()) + k) % 4]


def make_hap(ref, ref_start, edits=(), is_ref=False, loc=None, hap_start=0):
    """A haplotype over the whole reference from edits by reference index, ascending and apart: ("S", i, byte) a substitution,
    ("I", i, bytes) an insertion in front of base i, ("D", i, n) bases i .. i + n - 1 deleted."""
    bases, cigar, at = bytearray(), [], 0

    def m(n):
        if n:
            if cigar and cigar[-1][0] == R.OP_M:
                cigar[-1] = (R.OP_M, cigar[-1][1] + n)
            else:
                cigar.append((R.OP_M, n))

    for e in edits:
        kind, i = e[0], e[1]
        bases += ref[at:i]
        m(i - at)
        at = i
        if kind == "S":
            bases.append(e[2])
            m(1)
            at = i + 1
        elif kind == "I":
            bases += e[2]
            cigar.append((R.OP_I, len(e[2])))
        else:
            cigar.append((R.OP_D, e[2]))
            at = i + e[2]
    bases += ref[at:]
    m(len(ref) - at)
    return (bytes(bases), cigar, hap_start, loc or (ref_start, ref_start + len(ref) - 1), is_ref)


def snps(ref, idx):
    return [("S", i, other(ref[i])) for i in idx]


# ---- spans --------------------------------------------------------------------------------------------------------------------------
def span_set():
    rng = random.Random(11)
    ref = rand_ref(rng, 700)
    rs, active, padded = 1000, (1150, 1549), (1000, 1699)
    regions, names = [], []

    def add(name, haps, ref=ref, rs=rs, active=active, padded=padded):
        names.append(name)
        regions.append((ref, rs, active, padded, [make_hap(ref, rs, (), True)] + haps))

    for n in (0, 1, 63, 64, 65, 130):            # events of one haplotype: whole passes, one more, one less
        add("events_%d" % n, [make_hap(ref, rs, snps(ref, range(152, 152 + 3 * n, 3)))])
    for at in (63, 64):                          # the padded extreme on lane 63 of the first pass / lane 0 of the second
        ed = snps(ref, range(152, 152 + 3 * 65, 3))
        ed[at] = ("I", ed[at][1], b"GG")
        add("extreme_end_lane_%d" % at, [make_hap(ref, rs, ed)])
        ed = snps(ref, range(152, 152 + 3 * 65, 3))
        ed[at] = ("D", ed[at][1], 1)
        far = snps(ref, [160])                   # a second haplotype: its one event is lane 0 of its own pass
        add("extreme_both_lane_%d" % at, [make_hap(ref, rs, ed), make_hap(ref, rs, far)])
    add("deletion_only_ends_inside", [make_hap(ref, rs, [("D", 140, 15)])])          # 1139 .. 1154
    add("deletion_only_starts_inside", [make_hap(ref, rs, [("D", 545, 30)])])        # 1544 .. 1574
    add("deletion_encloses_active", [make_hap(ref, rs, [("D", 149, 402)])], active=(1150, 1549))
    add("event_in_padding_only", [make_hap(ref, rs, snps(ref, [20, 640]))])
    add("event_in_padding_and_inside", [make_hap(ref, rs, snps(ref, [20, 300, 640]))])
    add("event_at_active_edges", [make_hap(ref, rs, snps(ref, [150, 549]))])
    add("event_just_outside_active", [make_hap(ref, rs, snps(ref, [149, 550]))])
    add("snp_only", [make_hap(ref, rs, snps(ref, [300, 310]))])
    add("snp_and_one_indel", [make_hap(ref, rs, snps(ref, [300]) + [("I", 310, b"T")])])
    add("mnp", [make_hap(ref, rs, snps(ref, [300, 301, 302]))])
    add("snp_joined_with_insertion_stays_a_snp", [make_hap(ref, rs, [("S", 300, other(ref[300])), ("I", 301, b"TT")])])
    return dict(regions=regions, names=names, dist=0, padding=SMALL)


def edge_span_set():
    """The reference's default paddings against the region's padded span, a start smaller than its padding, the repeat slice."""
    rng = random.Random(12)
    ref = rand_ref(rng, 400)
    regions, names = [], []

    def add(name, rs, active, padded, edits, ref=ref):
        names.append(name)
        regions.append((ref, rs, active, padded, [make_hap(ref, rs, (), True), make_hap(ref, rs, edits)]))

    add("start_smaller_than_padding", 0, (2, 300), (0, 399), snps(ref, [4]))
    add("start_smaller_than_padding_indel", 3, (10, 300), (3, 402), [("I", 30, b"A")])
    add("padding_cut_left", 1000, (1050, 1300), (1040, 1399), snps(ref, [55]))
    add("padding_cut_right", 1000, (1050, 1300), (1000, 1310), snps(ref, [295]))
    add("padding_cut_both", 1000, (1050, 1300), (1045, 1305), [("D", 100, 3), ("I", 250, b"CC")])
    add("padding_not_cut", 1000, (1100, 1250), (1000, 1399), snps(ref, [180]))
    add("active_is_padded", 1000, (1000, 1399), (1000, 1399), snps(ref, [0, 399]))
    add("one_base_active", 1000, (1200, 1200), (1200, 1200), snps(ref, [200]))
    # an indel that starts more than one base in front of the padded span: the repeat slice underflows
    add("repeat_slice_underflow", 1000, (1150, 1300), (1100, 1350), [("D", 90, 70)])
    add("repeat_slice_at_the_edge", 1000, (1150, 1300), (1100, 1350), [("D", 100, 60)])   # start 1099: index 0, fine
    add("snp_in_front_of_the_padded_span_is_no_slice", 1000, (1150, 1300), (1100, 1350), snps(ref, [200]))
    return dict(regions=regions, names=names, dist=0, padding=DEFAULT)


# ---- Haplotype::trim ----------------------------------------------------------------------------------------------------------------
EXH_REF = b"ACGTTGCATGCAAGTC"
EXH_START = 100


def cigar_hap(cigar, ref, ins=b"G"):
    """the bases a CIGAR spells over ref from index 0: the reference under M, `ins` under I"""
    bases, at = bytearray(), 0
    for op, n in cigar:
        if op == R.OP_M:
            bases += ref[at:at + n]
            at += n
        elif op == R.OP_I:
            bases += ins * n
        else:
            at += n
    return bytes(bases), at


def exhaustive_cigars(max_elements=4, max_len=3):
    elements = [(op, n) for op in (R.OP_M, R.OP_I, R.OP_D) for n in range(1, max_len + 1)]
    for k in range(1, max_elements + 1):
        for c in itertools.product(elements, repeat=k):
            yield list(c)


def exhaustive_set(max_elements=4, max_len=3):
    """Every CIGAR of up to max_elements elements over {M, I, D} with lengths 1 .. max_len against every (start, stop) inside
    its reference length.  All haplotypes share the region's reference coordinates (hap_start 0) and differ in their LOCATION,
    which is what Haplotype::trim measures new_start from; a region is one width stop - start, its padded span starts at the
    reference's first base (no repeat slice can underflow), one more haplotype carries the SNP that makes the variation.
    CIGARs whose event map fails (two insertions at one start) would fail the whole region: they go into regions of their own."""
    import events_restatement as EV
    by_width, failing = {}, []
    for cigar in exhaustive_cigars(max_elements, max_len):
        bases, ref_len = cigar_hap(cigar, EXH_REF)
        try:
            EV.event_map(EXH_REF, EXH_START, bases, cigar, 0, 0)
            ok = True
        except EV.Panic:
            ok = False
        for start in range(ref_len):
            for stop in range(start, ref_len):
                hap = (bases, cigar, 0, (EXH_START - start, EXH_START - start + ref_len - 1), False)
                (by_width.setdefault(stop - start, []) if ok else failing).append((hap, stop - start))
    snp = (bytes([other(EXH_REF[0])]) + EXH_REF[1:], [(R.OP_M, len(EXH_REF))], 0, (EXH_START, EXH_START + len(EXH_REF) - 1), False)
    regions = []
    for w, haps in sorted(by_width.items()):
        for i in range(0, len(haps), 511):
            regions.append((EXH_REF, EXH_START, (EXH_START, EXH_START + w), (EXH_START, EXH_START + w), [snp] + [h for h, _ in haps[i:i + 511]]))
    for hap, w in failing[::37]:     # (the event map is the same whatever the span: a sample of them, one a region)
        regions.append((EXH_REF, EXH_START, (EXH_START, EXH_START + w), (EXH_START, EXH_START + w), [snp, hap]))
    return dict(regions=regions, dist=0, padding=DEFAULT)


def trim_edge_set():
    """A 200-element CIGAR; spans that end one past the CIGAR's reference length (the two tests behind the loop, min(stop + 1,
    len)); a location longer than the CIGAR; every status family."""
    rng = random.Random(13)
    ref = rand_ref(rng, 300)
    rs = 1000
    regions, names = [], []
    def add(name, span, haps, ref=ref):
        names.append(name)
        regions.append((ref, rs, span, span, [make_hap(ref, rs, snps(ref, [span[0] - rs]))] + haps))   # the SNP that makes the variation

    long_cigar = [(R.OP_M, 2), (R.OP_I, 1), (R.OP_M, 2), (R.OP_D, 1)] * 50   # 200 elements, 250 reference bases
    bases, ref_len = cigar_hap(long_cigar, ref, b"T")
    long_hap = (bases, long_cigar, 0, (rs, rs + ref_len - 1), False)
    for span in ((rs, rs + 249), (rs + 1, rs + 248), (rs + 3, rs + 7), (rs + 4, rs + 240), (rs, rs + 4), (rs + 100, rs + 101)):
        add("long_cigar_%d_%d" % span, span, [long_hap])
    short = cigar_hap([(R.OP_M, 10)], ref)[0]
    wide = (rs, rs + 40)
    add("stop_one_past_the_cigar", (rs + 4, rs + 10), [(short, [(R.OP_M, 10)], 0, wide, False)])
    add("start_and_stop_one_past_the_cigar", (rs + 10, rs + 10), [(short, [(R.OP_M, 10)], 0, wide, False)])
    add("stop_one_past_behind_an_insertion", (rs + 4, rs + 10), [(short + b"GG", [(R.OP_M, 10), (R.OP_I, 2)], 0, wide, False)])
    add("stop_one_past_behind_a_deletion", (rs + 4, rs + 12), [(short, [(R.OP_M, 10), (R.OP_D, 2)], 0, wide, False)])
    add("hap_start_is_carried", (rs + 4, rs + 8), [(short, [(R.OP_M, 10)], 7, wide, False)])
    add("all_insertion", (rs + 10, rs + 10), [(short + b"G", [(R.OP_M, 10), (R.OP_I, 1)], 0, wide, False)])
    # -- the status families, each beside a healthy region (the callers put them into one batch)
    add("status_LOCATION_left", (rs + 2, rs + 8), [(short, [(R.OP_M, 10)], 0, (rs + 3, rs + 12), False)])
    add("status_LOCATION_right", (rs + 2, rs + 8), [(short, [(R.OP_M, 10)], 0, (rs, rs + 7), False)])
    add("status_LENGTH", (rs + 2, rs + 8), [(short + b"A", [(R.OP_M, 10)], 0, wide, False)])
    add("status_OPERATOR", (rs + 2, rs + 8), [(b"GG" + short, [(R.OP_S, 2), (R.OP_M, 10)], 0, wide, False)])
    add("operator_behind_the_stop_is_not_reached", (rs + 2, rs + 8), [(short + b"GG", [(R.OP_M, 10), (R.OP_S, 2)], 0, wide, False)])
    add("status_NOT_FOUND", (rs + 2, rs + 20), [(short, [(R.OP_M, 10)], 0, wide, False)])
    # a right soft clip with an insertion behind it, the span ending on the last matched base: the walk is done inside the M, the
    # trimmed CIGAR keeps the zero-length S at end + 1 and CigarBuilder::add refuses the I behind it ("Failed to add Cigar element")
    add("status_BUILDER", (rs + 2, rs + 9), [(short + b"GGTTT", [(R.OP_M, 10), (R.OP_S, 2), (R.OP_I, 3)], 0, wide, False)])
    add("clip_and_insertion_behind_the_stop_are_not_reached", (rs + 2, rs + 8), [(short + b"GGTTT", [(R.OP_M, 10), (R.OP_S, 2), (R.OP_I, 3)], 0, wide, False)])
    add("status_REF_ELIMINATED", (rs + 2, rs + 6), [(short[:5] + short[7:], [(R.OP_M, 5), (R.OP_D, 2), (R.OP_M, 3)], 0, wide, True)])
    add("cut_in_deletion_of_a_non_reference", (rs + 2, rs + 5), [(short[:5] + short[7:], [(R.OP_M, 5), (R.OP_D, 2), (R.OP_M, 3)], 0, wide, False)])
    add("first_panic_in_input_order_wins", (rs + 2, rs + 8), [(short + b"A", [(R.OP_M, 10)], 0, wide, False),
                                                              (short, [(R.OP_M, 10)], 0, (rs + 3, rs + 12), False)])
    add("event_ALLELES", (rs + 2, rs + 8), [(short[:4] + short[4:5].lower() + short[5:], [(R.OP_M, 10)], 0, wide, False)])
    add("event_BAD_OPERATOR", (rs + 2, rs + 8), [(short, [(R.OP_M, 5), (R.OP_N, 2), (R.OP_M, 5)], 0, wide, False)])
    add("event_BLOCK", (rs + 2, rs + 8), [(short + b"GG", [(R.OP_M, 5), (R.OP_I, 1), (R.OP_I, 1), (R.OP_M, 5)], 0, wide, False)])
    add("event_CIGAR_OVERRUN", (rs + 2, rs + 8), [(short, [(R.OP_M, 12)], 0, wide, False)])
    add("healthy_beside_them", (rs + 2, rs + 8), [(short, [(R.OP_M, 10)], 0, wide, False)])
    return dict(regions=regions, names=names, dist=0, padding=DEFAULT)


# ---- order and duplicates -----------------------------------------------------------------------------------------------------------
def order_set():
    rng = random.Random(14)
    ref = rand_ref(rng, 300)
    rs, active, padded = 1000, (1100, 1199), (1000, 1299)   # SNPs at both active edges: the trimmed window is 1080 .. 1219, 140 bases
    regions, names = [], []
    edge = [100, 199]

    def add(name, haps, ref=ref):
        names.append(name)
        regions.append((ref, rs, active, padded, haps))

    def hap(idx, is_ref=False, r=ref):
        return make_hap(r, rs, snps(r, sorted(set(idx))), is_ref)

    for n in (1, 2, 63, 64, 65, 128, 512):       # distinct haplotypes, duplicates among them, shuffled
        pool = [hap(edge + [101 + (i * 7) % 97, 102 + (i * 11) % 89]) for i in range(n)]
        rng.shuffle(pool)
        add("haplotypes_%d" % n, pool)
    add("differ_only_outside_the_padded_span", [hap(edge + [i]) for i in (5, 30, 60, 79, 220, 250, 290)] + [hap(edge)])
    same = [hap(edge + [150]) for _ in range(4)]
    for at, name in ((0, "first"), (2, "middle"), (3, "last")):
        members = [(h[0], h[1], h[2], h[3], i == at) for i, h in enumerate(same)]
        add("reference_%s_in_its_class" % name, [hap(edge + [120])] + members + [hap(edge + [170])])
    add("two_references_in_one_class", [(h[0], h[1], h[2], h[3], i in (1, 3)) for i, h in enumerate(same)] + [hap(edge + [120])])
    # a shorter haplotype with larger bytes, a longer one with smaller bytes
    low, high = bytes([min(BASES)]), bytes([max(BASES)])
    add("length_before_bytes", [make_hap(ref, rs, snps(ref, edge)),
                                make_hap(ref, rs, [("S", 100, other(ref[100])), ("S", 110, high[0] if ref[110] != high[0] else BASES[2]), ("D", 150, 3), ("S", 199, other(ref[199]))]),
                                make_hap(ref, rs, [("S", 100, other(ref[100])), ("I", 150, low * 2), ("S", 199, other(ref[199]))]),
                                make_hap(ref, rs, (), True)])
    # a first difference at byte 63, 64, 65, 128 and at the last byte (139) of the trimmed window, against equal prefixes
    for k in (63, 64, 65, 128, 139):
        third = sorted(snps(ref, edge) + [("S", 80 + k, other(ref[80 + k], 2))], key=lambda e: e[1])   # another base at the same place
        add("first_difference_at_%d" % k, [hap(edge), hap(edge + [80 + k]), make_hap(ref, rs, third)])
    # lower case against upper case: equal once upper-cased, so they fold; a lower-case base the reference shares comes out upper
    c = other(ref[150])
    low_ref = ref[:160] + ref[160:161].lower() + ref[161:]
    add("lower_case_folds_with_upper_case", [make_hap(low_ref, rs, [("S", 100, other(ref[100])), ("S", 150, c), ("S", 199, other(ref[199]))]),
                                             make_hap(low_ref, rs, [("S", 100, other(ref[100])), ("S", 150, bytes([c]).lower()[0]), ("S", 199, other(ref[199]))]),
                                             make_hap(low_ref, rs, (), True)], ref=low_ref)
    return dict(regions=regions, names=names, dist=0, padding=DEFAULT)


# ---- whole calls --------------------------------------------------------------------------------------------------------------------
def seeded_region(rng, n_haps=8, ref_len=300):
    ref = rand_ref(rng, ref_len)
    rs = rng.randrange(0, 5000)
    lo = rng.randrange(40, 100)
    hi = rng.randrange(ref_len - 100, ref_len - 40)
    pad = rng.randrange(0, 40)
    active, padded = (rs + lo, rs + hi), (rs + lo - pad, rs + hi + pad)
    haps = [make_hap(ref, rs, (), True)]
    pool = []
    for _ in range(n_haps - 1):
        edits, at = [], rng.randrange(2, 60)
        while at < ref_len - 8:
            kind = rng.choice("SSSID")
            if kind == "S":
                edits.append(("S", at, other(ref[at], rng.randrange(1, 4))))
            elif kind == "I":
                edits.append(("I", at, rand_ref(rng, rng.randrange(1, 4))))
            else:
                edits.append(("D", at, rng.randrange(1, 5)))
            at += rng.randrange(6, 90)
        pool.append(edits)
    for i, edits in enumerate(pool):
        haps.append(make_hap(ref, rs, pool[rng.randrange(i + 1)] if rng.random() < 0.2 else edits))
    rng.shuffle(haps)
    return (ref, rs, active, padded, haps)


def seeded_set(n=24, seed=15):
    rng = random.Random(seed)
    regions = [seeded_region(rng) for _ in range(n)]
    ref = rand_ref(rng, 120)
    regions.insert(5, (ref, 700, (720, 800), (700, 819), []))                                        # a region without haplotypes
    regions.insert(11, (ref, 700, (720, 800), (700, 819), [make_hap(ref, 700, (), True)] * 2))       # ... without variation
    return dict(regions=regions, dist=1, padding=SMALL)


def sets():
    return dict(spans=span_set(), edge_spans=edge_span_set(), trim_edges=trim_edge_set(), order=order_set(), seeded=seeded_set())
