"""The inputs of the finalize tests: test_finalize_oracle.py counts what they exercise on the restatement alone,
test_finalize_hip.py runs them on the device.  A case set is (name, groups, options): groups as finalize_restatement.finalize_reads
takes them, options its keyword arguments (steps, min_tail_quality, ...)."""
import json
import os
import random

import finalize_restatement as FR

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "read_clipper_cases.json")))
PAIRED, UNMAPPED, MATE_UNMAPPED, REVERSE, MATE_REVERSE = 0x1, 0x4, 0x8, 0x10, 0x20
FORWARD_PAIR, REVERSE_PAIR = PAIRED | MATE_REVERSE, PAIRED | REVERSE
FAR = 1 << 40


def cycle(values, n):
    return [values[i % len(values)] for i in range(n)]


def read(cigar, pos=None, flags=0, mapq=60, mpos=-1, isize=0, quals=None, bases=None, mate=-1):
    """a read of the CIGAR's length: the artificial read of the reference's tests unless told otherwise"""
    c = FR.parse_cigar(cigar) if isinstance(cigar, str) else cigar
    n = sum(l for op, l in c if FR.consumes_read(op))
    if isinstance(quals, int):
        quals = [quals] * n
    return dict(cigar=cigar, pos=GOLDEN["position"] if pos is None else pos, flags=flags, mapq=mapq, mpos=mpos, isize=isize,
                quals=list(quals) if quals is not None else cycle(GOLDEN["quals"], n),
                bases=bytes(bases) if bases is not None else bytes(cycle(GOLDEN["bases"].encode(), n)), mate=mate)


def group(reads, span=(0, FAR)):
    return dict(span=tuple(span), reads=list(reads))


def limits(cigar, pos):
    """(soft start, soft end) of a read: every coordinate a cut can fall on"""
    r = FR.Read(pos, 0, 60, -1, 0, cigar, 0)
    soft_end = r.get_end()
    for op, n in reversed(r.cigar):
        if op == FR.S:
            soft_end += n
        elif op != FR.H:
            break
    return r.get_soft_start_i64(), soft_end


def with_fragment(rd, reverse=False):
    """the read with a well-defined fragment size, so that its soft clips are reverted"""
    out = dict(rd)
    if reverse:
        out.update(flags=REVERSE_PAIR, mpos=rd["pos"] - 1, isize=-50)
    else:
        out.update(flags=FORWARD_PAIR, mpos=rd["pos"] + 20, isize=50)
    return out


def adaptor_reads(cigar, pos, coordinate):
    """the forward and the reverse read whose adaptor boundary is `coordinate`"""
    out = []
    if coordinate > pos:
        out.append(read(cigar, pos, FORWARD_PAIR, mpos=pos, isize=coordinate - pos, quals=30))
    out.append(read(cigar, pos, REVERSE_PAIR, mpos=coordinate + 1, isize=-30, quals=30))
    return out


def exhaustive():
    """the reference's CIGAR family (reads of 1 to 12 bases): each step alone and all steps together against every cut
    coordinate from the soft start to the soft end -- one call per step"""
    pos = GOLDEN["position"]
    cigars = GOLDEN["cigars"]
    sets = []
    plain = [read(c) for c in cigars]
    sets.append(("soft clips hard-clipped", [group(plain)], dict(steps=FR.FIN_SOFT_CLIPS, dont_use_soft_clipped_bases=True)))
    sets.append(("soft clips by fragment", [group(plain + [with_fragment(r) for r in plain] + [with_fragment(r, True) for r in plain])],
                 dict(steps=FR.FIN_SOFT_CLIPS)))
    tails = []
    for c in cigars:   # test_hard_clip_low_qual_ends: the three tail patterns
        n = len(read(c)["quals"])
        for low in range(n + 1):
            left, right = [2] * low + [30] * (n - low), [30] * (n - low) + [2] * low
            tails += [read(c, quals=left), read(c, quals=right)]
            if low <= n // 2:
                tails.append(read(c, quals=[2] * low + [30] * (n - 2 * low) + [2] * low))
    sets.append(("low-quality tails", [group(tails)], dict(steps=FR.FIN_LOW_QUAL_ENDS, min_tail_quality=2)))
    adaptor, region, everything = [], [], []
    for c in cigars:
        lo, hi = limits(c, pos)
        for i in range(lo, hi + 1):
            adaptor += adaptor_reads(c, pos, i)
            for span in ((i, FAR), (0, i), (i, min(i + 1, hi))):
                region.append(group([read(c, quals=30)], span))
                everything.append(group([read(c), with_fragment(read(c))], span))
    sets.append(("adaptor", [group(adaptor)], dict(steps=FR.FIN_ADAPTOR)))
    sets.append(("region", region, dict(steps=FR.FIN_REGION)))
    sets.append(("all steps", everything, dict(steps=FR.FIN_ALL, min_tail_quality=9)))
    return sets


def tail_scan():
    """window lengths around the scan's pass boundaries; the run of low-quality bases ends at, one before and one past each
    boundary, from either side; all low; low only at index 0"""
    reads = []
    for n in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300):
        runs = sorted({k for b in (0, 1, 16, 32, 48, 64, 128, 256, n) for k in (b - 1, b, b + 1) if 0 <= k <= n})
        for k in runs:
            reads.append(read("%dM" % n, quals=[3] * k + [40] * (n - k)))
            reads.append(read("%dM" % n, quals=[40] * (n - k) + [3] * k))
            reads.append(read("%dM" % n, quals=[3] * min(k, n // 2) + [40] * (n - min(k, n // 2) - k // 2) + [3] * (k // 2)))
        reads.append(read("%dM" % n, quals=[3] + [40] * (n - 1)))
        reads.append(read("%dM" % n, quals=[9] * n))
        reads.append(read("%dM" % n, quals=[40] * (n - 1) + [3]))
        if n > 4:   # a soft clip in front: the scan runs over the window the soft-clip step left
            reads.append(read("3S%dM" % (n - 3), quals=[40, 40, 40, 3] + [40] * (n - 4)))
            reads.append(read("2H3S%dM1S" % (n - 4), quals=[40, 40, 40, 3] + [40] * (n - 6) + [3, 40]))
    return [("tail scan", [group(reads)], dict(steps=FR.FIN_SOFT_CLIPS | FR.FIN_LOW_QUAL_ENDS, min_tail_quality=9,
                                                dont_use_soft_clipped_bases=True))]


def edges():
    reads = []
    # soft clips that revert to a start of 1, 0, -1, -10; the reference's before-contig cases
    for start in (1, 0, -1, -10):
        for pos in (1, 10):
            soft = "%dS" % (pos - start) if pos > start else ""
            reads.append(with_fragment(read(soft + "10M", pos, quals=30)))
            reads.append(with_fragment(read("2H" + soft + "10M3S1H", pos, quals=30)))
    for c in GOLDEN["before_contig"]:
        reads.append(with_fragment(read(c["cigar"], c["alignment_start"])))
    reads.append(with_fragment(read("12S3M", 2, quals=30)))            # loses more bases than it has left of the contig's start
    reads.append(with_fragment(read(GOLDEN["entirely_soft_clipped"])))
    reads.append(read(GOLDEN["entirely_soft_clipped"]))
    # hard clips outside soft clips; a read that is all clips; a read of length 0
    reads += [read("3H2S10M2S3H", quals=30), read("3H10M3H", quals=30), read("5S", quals=30), read("4H"), read([]), read("2H3S")]
    reads.append(read("5M", flags=UNMAPPED, quals=[2, 30, 30, 30, 30]))   # flagged unmapped: a hard clip leaves 0M
    # where the reference panics: a hard clip in the middle (the builder's Err is unwrapped); a CIGAR that ends in a deletion,
    # cut inside it from the right (Start > Stop)
    reads.append(read("5M2H5M", quals=[2] + [30] * 9))
    reads.append(read("5M3D", 100, FORWARD_PAIR, mpos=100, isize=6, quals=30))
    # a deletion or an insertion touching each cut
    for c in ("4M2D4M", "4M2I4M", "1M2D1M", "1M1I1M", "3S4M2D4M3S", "4M2D1I4M", "4M1I2D4M"):
        lo, hi = limits(c, 100)
        for i in range(lo, hi + 1):
            reads += adaptor_reads(c, 100, i)
    # CIGARs of 1, 2 and 200 elements
    long_cigar = "".join("%d%s" % (1 + k % 3, "MID"[0 if k % 2 == 0 else 1 + (k // 2) % 2]) for k in range(199)) + "2M"
    reads += [read("20M", quals=30), read("3S17M", quals=30), read(long_cigar, 500), with_fragment(read("4S" + long_cigar, 500))]
    n_long = len(read(long_cigar)["quals"])
    reads.append(read(long_cigar, 500, quals=[2] * 7 + [30] * (n_long - 12) + [2] * 5))
    groups = [group(reads)]
    # the adaptor step: forward and reverse; the boundary inside, at either end of and outside the read; isize 0; the mate
    # unmapped; the same strand; mpos 0 on a reverse read (the reference panics)
    adaptor = []
    for b in (90, 99, 100, 101, 110, 118, 119, 120, 130):
        adaptor += adaptor_reads("20M", 100, b)
    adaptor += [read("20M", 100, FORWARD_PAIR, mpos=100, isize=0, quals=30), read("20M", 100, FORWARD_PAIR | MATE_UNMAPPED, mpos=100, isize=10, quals=30),
                read("20M", 100, PAIRED, mpos=100, isize=10, quals=30), read("20M", 100, PAIRED | REVERSE | MATE_REVERSE, mpos=105, isize=-10, quals=30),
                read("20M", 100, isize=10, quals=30), read("20M", 100, REVERSE_PAIR, mpos=0, isize=-10, quals=30),
                read("20M", 0, REVERSE_PAIR, mpos=0, isize=-10, quals=30), read("20M", 100, REVERSE_PAIR, mpos=-1, isize=-10, quals=30),
                read("20M", 100, REVERSE_PAIR, mpos=1, isize=-10, quals=30), read("20M", 100, FORWARD_PAIR, mpos=100, isize=-10, quals=30),
                read("3S17M", 1, REVERSE_PAIR | UNMAPPED, mpos=5, isize=-10, quals=30)]
    groups.append(group(adaptor))
    # the region clip: inside, over the left edge, the right edge, both, outside either side; span start 0; a deletion at the edge
    for span in ((100, 200), (105, 200), (0, 110), (105, 110), (0, 50), (300, 400), (0, 0), (0, 99), (0, 100), (119, 119), (120, 125), (110, 110)):
        groups.append(group([read("20M", 100, quals=30), read("5M3D12M", 100, quals=30), read("3S14M3S", 100, quals=30)], span))
    for span in ((0, 104), (0, 105), (0, 106), (0, 107), (0, 108), (105, FAR), (106, FAR), (108, FAR), (109, FAR), (104, 109), (106, 107)):
        groups.append(group([read("5M3D12M", 100, quals=30), read("5M3D2I10M", 100, quals=30), read("5M2I3D10M", 100, quals=30)], span))
    groups.append(group([read("10M", 0, quals=30), read("2S8M", 0, quals=30)], (0, 5)))
    groups.append(group([]))
    return [("edges", groups, dict(steps=FR.FIN_ALL, min_tail_quality=9))]


def pair(first, second):
    """two reads that name each other, as the first two reads of a group"""
    a, b = dict(first), dict(second)
    a["mate"], b["mate"] = 1, 0
    return [a, b]


def mates(cigar_a, pos_a, cigar_b, pos_b, quals_a=30, quals_b=30, bases_a=None, bases_b=None, **more):
    return pair(read(cigar_a, pos_a, PAIRED, mpos=pos_b, isize=0, quals=quals_a, bases=bases_a, **more),
                read(cigar_b, pos_b, PAIRED | REVERSE, mpos=pos_a, isize=0, quals=quals_b, bases=bases_b, **more))


def pairs():
    groups = []
    n = 100
    acgt = bytes(cycle(b"ACGT", n))
    for overlap in (1, 63, 64, 65, 100):   # overlapping by 1, 63, 64, 65 and all bases, bases agreeing
        shift = n - overlap
        b = bytes(cycle(b"ACGT", n + shift))[shift:]
        groups.append(group(mates("100M", 1000, "100M", 1000 + shift, bases_a=acgt, bases_b=b, quals_a=[10, 35] * 50, quals_b=[35, 10, 20, 21] * 25)))
        wrong = bytearray(b)
        for k in range(0, n, 7):
            wrong[k] = ord("N")
        groups.append(group(mates("100M", 1000, "100M", 1000 + shift, bases_a=acgt, bases_b=bytes(wrong), quals_a=[10, 35] * 50, quals_b=40)))
    groups.append(group(mates("50M", 1000, "50M", 1000)))                                  # equal soft starts: the second is the first
    groups.append(group(mates("50M", 1000, "5S45M", 1005)))
    groups.append(group(mates("20M10D20M", 1000, "30M", 1025)))                            # the second starts inside a deletion
    groups.append(group(mates("30M10S", 1000, "30M", 1032)))  # ... inside a soft clip of the first
    groups.append(group(mates("30M", 1000, "30M", 1030)))                                  # adjacent, no overlap
    groups.append(group(mates("30M", 1000, "30M", 1029)))
    groups.append(group(mates("10M5I15M", 1000, "5S25M", 1010)))
    groups.append(group(mates("30M", 1000, "30M", 1010, quals_a=9, quals_b=30)))          # a mate the low-quality step removes
    groups.append(group(mates("30M", 1000, "30M", 2000), (0, 1500)))                       # a mate the region removes
    groups.append(group([read("30M", 1000, PAIRED, mpos=1010, quals=30), read("30M", 1010, PAIRED | REVERSE, mpos=1000, quals=30)]))   # mate_index -1
    groups.append(group(pair(read("30M", 1000, PAIRED, mpos=-1, quals=30), read("30M", 1010, PAIRED, mpos=1000, quals=30))))
    groups.append(group(pair(read("30M", 1000, PAIRED, mpos=1031, quals=30), read("30M", 1010, PAIRED, mpos=1000, quals=30))))
    groups.append(group(pair(read("30M", 1000, 0, mpos=1010, quals=30), read("30M", 1010, PAIRED, mpos=1000, quals=30))))
    groups.append(group(pair(read("30M", 1000, PAIRED | MATE_UNMAPPED, mpos=1010, quals=30), read("30M", 1010, PAIRED, mpos=1000, quals=30))))
    # the comparator's keys one after the other: equal starts, then strand, flags, mapq, mpos, length, index
    same = dict(quals_a=[25, 15] * 10, quals_b=[15, 25] * 10)
    groups.append(group(pair(read("20M", 1000, PAIRED | REVERSE, mpos=1000, quals=25), read("20M", 1000, PAIRED, mpos=1000, quals=15))))
    groups.append(group(pair(read("20M", 1000, PAIRED | 0x80, mpos=1000, quals=25), read("20M", 1000, PAIRED | 0x40, mpos=1000, quals=15))))
    groups.append(group(pair(read("20M", 1000, PAIRED, 50, mpos=1000, quals=25), read("20M", 1000, PAIRED, 40, mpos=1000, quals=15))))
    groups.append(group(pair(read("20M", 1000, PAIRED, mpos=1001, quals=25), read("20M", 1000, PAIRED, mpos=1000, quals=15))))
    groups.append(group(pair(read("21M", 1000, PAIRED, mpos=1000, quals=25), read("20M", 1000, PAIRED, mpos=1000, quals=15))))
    groups.append(group(mates("20M", 1000, "20M", 1000, **same)))
    # soft starts that differ although the starts are equal, in either input order
    groups.append(group(pair(read("3S20M", 1000, PAIRED, mpos=1000, quals=30), read("20M", 1000, PAIRED, mpos=1000, quals=30))))
    groups.append(group(pair(read("20M", 1000, PAIRED, mpos=1000, quals=30), read("3S20M", 1000, PAIRED, mpos=1000, quals=30))))
    # several pairs and singletons in one group, mates far apart in input order
    many = []
    for k in range(6):
        many += [read("40M", 5000 + 7 * k, PAIRED, mpos=5020 + 7 * k, quals=[12, 33] * 20), read("25M", 4000 + k, quals=30)]
    for k in range(6):
        many.append(read("40M", 5020 + 7 * k, PAIRED | REVERSE, mpos=5000 + 7 * k, quals=[33, 12] * 20, bases=bytes(cycle(b"ACTGA", 40))))
        many[2 * k]["mate"], many[-1]["mate"] = len(many) - 1, 2 * k
    groups.append(group(many))
    return [("pairs", groups, dict(steps=FR.FIN_REGION | FR.FIN_LOW_QUAL_ENDS | FR.FIN_PAIRS, min_tail_quality=9, half_of_pcr_snv_qual=20)),
            ("pairs after soft clips", groups, dict(steps=FR.FIN_ALL, min_tail_quality=9, half_of_pcr_snv_qual=30, dont_use_soft_clipped_bases=True))]


def pair_panics():
    """pairs on which the reference's pair step panics, beside one it adjusts: a soft start below 0 (the read starts at 1 with 3
    soft clips, and the soft-clip step is not run), so get_soft_start().unwrap() fails; a second read that is one insertion, so
    no read index belongs to its end and the unwrap meets None"""
    groups = [group(pair(read("3S20M", 1, PAIRED, mpos=5, quals=30), read("20M", 5, PAIRED | REVERSE, mpos=1, quals=30))),
              group(mates("30M", 1000, "30M", 1010)),
              group(mates("30M", 1000, "5I", 1010) + [read("30M", 1000, quals=30)])]
    return [("pair panics", groups, dict(steps=FR.FIN_PAIRS))]


def random_set(seed, n_reads=2000, n_groups=40):
    """what an aligner emits, roughly: reads of 30 to 151 bases, leading / trailing soft clips, an indel now and then,
    low-quality tails, mates that overlap in about a third of the fragments"""
    rng = random.Random(seed)
    groups = []
    per = n_reads // n_groups
    for g in range(n_groups):
        start = rng.randrange(1, 5) * 1000 if g else 60    # the first group lies at the contig's start
        span = (start, start + 400)
        reads = []
        while len(reads) < per:
            n = rng.choice((30, 75, 100, 150, 151))
            lead = rng.choice((0, 0, 0, 1, 5, 20)) if n > 60 else 0
            trail = rng.choice((0, 0, 0, 2, 10)) if n > 60 else 0
            hard = rng.choice((0, 0, 0, 3))
            core = n - lead - trail
            kind = rng.choice("MMMMMID")
            if kind == "M" or core < 20:
                middle = "%dM" % core
            else:
                at, k = rng.randrange(5, core - 10), rng.randrange(1, 5)
                middle = "%dM%dD%dM" % (at, k, core - at) if kind == "D" else "%dM%dI%dM" % (at, k, core - at - k)
            cigar = ("%dH" % hard if hard else "") + ("%dS" % lead if lead else "") + middle + ("%dS" % trail if trail else "") + ("%dH" % hard if hard and rng.random() < 0.5 else "")
            pos = max(start - 100 + rng.randrange(0, 560), 0)
            quals = [rng.choice((2, 8, 12, 25, 30, 37, 40)) if rng.random() < 0.1 else rng.randrange(20, 41) for _ in range(n)]
            for side in (0, 1):
                k = rng.choice((0, 0, 1, 3, 12))
                if side:
                    quals[n - k:] = [rng.randrange(0, 9) for _ in range(k)]
                else:
                    quals[:k] = [rng.randrange(0, 9) for _ in range(k)]
            bases = bytes(rng.choice(b"ACGT") for _ in range(n))
            what = rng.random()
            if what < 0.25 or len(reads) + 2 > per:      # a single read
                reads.append(read(cigar, pos, rng.choice((0, REVERSE)), rng.randrange(0, 61), quals=quals, bases=bases))
                continue
            # a fragment: in about a third of them the mates overlap
            gap = rng.randrange(-n + 5, 0) if rng.random() < 0.45 else rng.randrange(0, 300)
            fragment_end = pos + n + gap + n
            mate_pos = max(pos + n + gap - lead, 0)
            a = read(cigar, pos, FORWARD_PAIR | 0x40, rng.randrange(20, 61), mpos=mate_pos, isize=fragment_end - pos, quals=quals, bases=bases)
            mate_bases = bytes(bases[(mate_pos - pos + i)] if 0 <= mate_pos - pos + i < n and rng.random() < 0.97 else rng.choice(b"ACGT") for i in range(n))
            b = read("%dM" % n, mate_pos, REVERSE_PAIR | 0x80, rng.randrange(20, 61), mpos=pos, isize=-(fragment_end - pos),
                     quals=[rng.randrange(10, 41) for _ in range(n)], bases=mate_bases)
            a["mate"], b["mate"] = len(reads) + 1, len(reads)
            reads += [a, b]
        order = list(range(len(reads)))
        rng.shuffle(order)                               # the input order is the caller's, not the sort's
        where = {old: new for new, old in enumerate(order)}
        shuffled = [dict(reads[old]) for old in order]
        for rd in shuffled:
            rd["mate"] = where[rd["mate"]] if rd["mate"] >= 0 else -1
        groups.append(group(shuffled, span))
    return [("random %d" % seed, groups, dict(steps=FR.FIN_ALL, min_tail_quality=9))]


RANDOM_SEEDS = (20261, 20262)


def all_sets():
    out = exhaustive() + tail_scan() + edges() + pairs() + pair_panics()
    for seed in RANDOM_SEEDS:
        out += random_set(seed)
    return out


_SETS, _RESTATED = [], {}


def sets():
    """all_sets(), made once"""
    if not _SETS:
        _SETS.extend(all_sets())
    return _SETS


def case(name):
    return next(c for c in sets() if c[0] == name)


def restated(name):
    """the restatement's results for a set, computed once and shared"""
    if name not in _RESTATED:
        _, groups, options = case(name)
        _RESTATED[name] = FR.finalize_reads(groups, **options)
    return _RESTATED[name]
