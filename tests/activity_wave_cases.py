"""Test infrastructure: windows that take phmm_activity_profile past the first trip of its lane-strided loops and onto the edges
of its dispatches, in the (name, windows, options) form of tests/activity_cases.py, restated once per process.
tests/test_activity_wave_table.py (CPU) counts what they cross and checks the witnesses; tests/test_activity_wave_hip.py (GPU)
holds the kernels to the restatement on them.

  long()      one read per window: M / = / X / D / S elements around 64 and 128 bases, elements that start before the window
              (j0 > 0) or run over its end with more than 64 bases inside, an I element's slot joined by a long M
  clips()     soft clips of 63 ... 130 bases, leading and trailing, all of high quality or only from clip offset 64 on
  threshold() a running average that reaches 6.0 through clip bases at offsets >= 64 alone, and the same reads without them
  seeded()    random windows under reads with elements of 1 ... 200 bases and clips of 0 ... 130, G = 4, 8, 9, 16, 17
  routes()    pairs of calls on one window, a sample count on either side of af_is_block_event
  grids()     n_pos and max_prof_n + max_filter_size around a multiple of 256
  quals()     a QUAL far above 255 and QUALs not above 0

A witness (WITNESS[name], a list of dicts) names a window position whose restated values a kernel that stopped after a loop's
first trip could not give: see `long_witness` and `clip_witness`."""
import functools
import random
from collections import Counter

import activity_cases as K
import activity_restatement as R

LANES = 64           # one wave per read: every loop of activity_read_kernel strides by it
START, CONTIG = 5000, 100000
WITNESS = {}


def trips(n):
    """How often a loop `for (j = lane; j < n; j += 64)` runs its body in at least one lane."""
    return (n + LANES - 1) // LANES


def elements(read, start, end):
    """(op, length, j0, j1, position of its first base) of each M / = / X / D element as parse_record walks it inside
    [start, end): the element's bases [j0, j1) get a pileup entry.  An I element at or past `end` ends the read."""
    pos = read[0]
    for op, n in R.parse_cigar(read[1]):
        if op in "M=XD":
            j0, j1 = min(max(start - pos, 0), n), min(max(end - pos, 0), n)
            yield op, n, j0, j1, pos
            pos += j1
        elif op == "I" and pos >= end:
            return


def pileup(window, ploidy=2):
    """The restated pileup of a window alone: (per sample [RefVsAnyResult], [RunningAverage])."""
    start, ref, contig, samples = window
    return R.update_activity_profile([[R.Record(*r) for r in reads] for reads in samples], ref, start, len(ref), contig, ploidy, K.BQ)


def other_base(b):
    return K.BASES[(K.BASES.index(bytes([b]).upper()) + 1) % 4]


# ---- a. long elements, one read per window ---------------------------------------------------------------------------------------

def long_witness(name, at, changed, second_trip):
    """Position `at` of the case's window is covered by its read alone; `changed` is the same window with one base of the read
    (or the one element) altered so that the entry at `at` is another one; second_trip: the entry's element offset is
    >= j0 + 64."""
    WITNESS.setdefault(name, []).append(dict(kind="long", at=at, changed=changed, second_trip=second_trip))


def _one(name, pos, cigar, ref, quals=None):
    return K.one_read(name, pos, cigar, ref, start=START, contig=CONTIG, quals=quals)


def _with_read(case, read):
    start, ref, contig, _ = case[1][0]
    return (start, ref, contig, [[read]])


def _mismatch_at(case, at):
    """The case's window with the read base that lies on window position `at` turned into a mismatch."""
    pos, cigar, bases, quals = case[1][0][3][0][0]
    ref_at, q = pos, 0
    for op, n in R.parse_cigar(cigar):
        if op in "M=X":
            if ref_at <= START + at < ref_at + n:
                q += START + at - ref_at
                b = bytearray(bases)
                b[q] = other_base(b[q])
                return _with_read(case, (pos, cigar, bytes(b), quals))
            ref_at, q = ref_at + n, q + n
        elif op == "D":
            ref_at += n
        elif op in "IS":
            q += n
    raise ValueError((case[0], at))


def long():
    ref = K.reference(random.Random(21), 420)
    out = []

    def match(name, pos, cigar, at, offset):
        """offset: the witness's distance from the element's first base inside the window (its element offset less j0)."""
        c = _one(name, pos, cigar, ref)
        out.append(c)
        long_witness(name, at, _mismatch_at(c, at), offset >= LANES)

    def deletion(name, pos, before, n, after, at, offset, j0=0):
        """`before`M `n`D `after`M; the changed window's deletion stops one base short of the witness, where a base of Q35
        stands instead (the deletion's entry is alt at Q30)."""
        c = _one(name, pos, "%dM%dD%dM" % (before, n, after), ref)
        out.append(c)
        rest = after + n - j0 - offset
        cut = _one(name, pos, "%dM%dD%dM" % (before, j0 + offset, rest), ref, quals=[35] * (before + rest))
        long_witness(name, at, cut[1][0], offset >= LANES)

    for op in "M=X":
        for n in (63, 64, 65, 128, 129, 200):
            match("long %d%s" % (n, op), START + 10, "%d%s" % (n, op), 10 + n - 1, n - 1)
    for n in (64, 65, 130):
        deletion("long %dD" % n, START + 10, 10, n, 10, 20 + n - 1, n - 1)
    # an I element's slot at the position of a long M's first base: the M joins it, and the table points at the I's slot
    match("63M2I66M", START + 10, "63M2I66M", 10 + 63 + 65, 65)
    match("5S128M3I64M70S", START + 10, "5S128M3I64M70S", 10 + 100, 100)
    # elements that start before the window: j0 > 0, and more than 64 of their bases remain
    match("200M from 70 before the window", START - 70, "200M", 129, 129)
    match("170M from 70 before the window", START - 70, "170M", 99, 99)
    deletion("200D from 70 before the window", START - 75, 5, 200, 20, 129, 129, j0=70)
    deletion("130D at the window's first position behind 70M", START - 70, 70, 130, 20, 129, 129)
    # ... and that run over bound_end with more than 64 bases inside
    match("200M over the window's end", START + 320, "200M", 419, 99)
    match("300X over the window's end", START + 270, "300X", 419, 149)
    deletion("150D over the window's end", START + 310, 10, 150, 10, 419, 99)
    return out


# ---- a. long soft clips ----------------------------------------------------------------------------------------------------------

CLIP_LENGTHS = (63, 64, 65, 130)
HIGH, LOW = 35, 20  # on either side of HQ_BASE_QUALITY_SOFTCLIP_THRESHOLD = 28; LOW is still counted (>= BQ)


def clip_witness(name, at, count, first_trip_alone):
    """soft_clip_mean at window position `at` is `count`, from one observation; a loop that stopped after the clip's first 64
    bases would have counted `first_trip_alone`."""
    WITNESS.setdefault(name, []).append(dict(kind="clip", at=at, count=count, first_trip_alone=first_trip_alone))


def clip_quals(n, late_only):
    return [LOW if late_only and k < LANES else HIGH for k in range(n)]


def clips():
    """The base beside a clip is alt (next to a soft clip) and adds the read's count to its position's running average."""
    ref = K.reference(random.Random(22), 120)
    out = []
    for n in CLIP_LENGTHS:
        for late_only in (False, True):
            count = max(n - LANES, 0) if late_only else n
            first = 0 if late_only else min(n, LANES)
            tag = "%dS %s" % (n, "high only from offset 64" if late_only else "all high")
            name = "leading " + tag
            bases = b"G" * n + ref[40:70]
            out.append(K.one_read(name, START + 40, "%dS30M" % n, ref, start=START, contig=CONTIG, bases=bases, quals=clip_quals(n, late_only) + [30] * 30))
            clip_witness(name, 40, count, first)
            name = "trailing " + tag  # align_pos is 30 at the clip's first base
            bases = ref[40:70] + b"C" * n
            out.append(K.one_read(name, START + 40, "30M%dS" % n, ref, start=START, contig=CONTIG, bases=bases, quals=[30] * 30 + clip_quals(n, late_only)))
            clip_witness(name, 69, count, first)
    return out


def threshold_window(late_qual, n_reads=5, length=150, seed=23):
    """`n_reads` reads 70S30M with a mismatch at their first aligned base; the clip's first 64 bases are LOW, its last six
    `late_qual`: with HIGH every read counts 6, the running average is 6.0 and the position's state is emitted 13 times."""
    ref = K.reference(random.Random(seed), length)
    bases = b"G" * 70 + bytes([other_base(ref[60])]) + ref[61:90]
    quals = [LOW] * LANES + [late_qual] * 6 + [35] * 30
    return (START, ref, CONTIG, [[(START + 60, "70S30M", bases, quals)] * n_reads])


THRESHOLD_AT = 60


def threshold():
    return [("average 6.0 from clip offsets >= 64 alone", [threshold_window(HIGH)], K.options()),
            ("the same reads, those six bases low", [threshold_window(LOW)], K.options())]


# ---- c. seeded windows under long reads --------------------------------------------------------------------------------------

def long_cigar(rng):
    """As activity_cases.random_cigar, with elements of 1 ... 200 bases and clips of 0 ... 130."""
    body, left = [], rng.randint(40, 320)
    lead = rng.choice([0, 0, 3, 63, 64, 65, 100, 130])
    trail = rng.choice([0, 0, 5, 63, 64, 65, 90, 130])
    if rng.random() < 0.1:
        body.append(("I", rng.randint(1, 3)))
    while left > 0:
        n = min(left, rng.choice([rng.randint(1, 200), rng.randint(60, 135)]))
        body.append((rng.choice("MMMM=XD") if body and body[-1][0] in "M=XI" and left > n else rng.choice("MMMM=X"), n))
        left -= n
        if left > 0 and rng.random() < 0.5:
            body.append((rng.choice("IDD") if body[-1][0] != "D" else "I", rng.randint(1, 5)))
    return ([("H", 3)] if rng.random() < 0.1 else []) + ([("S", lead)] if lead else []) + body + ([("S", trail)] if trail else [])


def seeded_window(seed, n_samples, start=START, length=420, contig=CONTIG, max_reads=20):
    rng = random.Random(seed)
    ref = K.reference(rng, length)
    samples = []
    for _ in range(n_samples):
        n = rng.randint(max_reads // 2, max_reads)
        pos = sorted(rng.randint(max(0, start - 150), start + length - 1) for _ in range(n))
        samples.append([K.read_for(rng, p, long_cigar(rng), start, ref) for p in pos])
    return (start, ref, contig, samples)


# samples, ploidy, profile size, positions, seed: G = 4, 8, 9, 16, 17
SEEDED = [(1, 3, 0, 420, 501), (2, 7, 128, 420, 502), (3, 8, 0, 300, 503), (2, 15, 200, 420, 504), (1, 16, 0, 300, 505), (3, 16, 128, 200, 506)]
REPEATED = "seeded long s2 p7 c128"  # with windows of its own beside it: test_activity_wave_hip.py's repeatability test


def seeded():
    return [("seeded long s%d p%d c%d" % c[:3], [seeded_window(c[4], c[0], length=c[3])], K.options(c[1], c[2])) for c in SEEDED]


def repeated_windows():
    """The windows of REPEATED and three more of its shape: a call over all of them against the windows one by one."""
    first = next(c for c in seeded() if c[0] == REPEATED)
    return first[1] + [seeded_window(520 + i, 2, start=300 * i, length=90 + 37 * i, contig=4000, max_reads=6) for i in range(3)], first[2]


# ---- d. the allele-frequency step's two routes ---------------------------------------------------------------------------------

AF_BLOCK_PASSES = 8  # phmm_af_internal.hpp; tests/test_activity_wave_table.py reads it there


def af_is_block_event(G, n_samples):
    """phmm_af.cpp: a sample takes S lanes (the next power of two >= G, 64 from G = 65 on); an event whose samples need eight
    or more passes of one wave goes to a whole workgroup."""
    S = 64
    if G <= 64:
        S = 1
        while S < G:
            S <<= 1
    per_pass = 64 // S
    return (n_samples + per_pass - 1) // per_pass >= AF_BLOCK_PASSES


ROUTE_PAIRS = [(32, 7, 8, 24, 531), (64, 7, 8, 12, 532), (4, 56, 57, 40, 533)]  # ploidy, samples on the wave route, on the block route, positions, seed


def route_window(seed, n_samples, length):
    """A few short reads per sample; sample s is the same reads whatever n_samples is."""
    rng = random.Random(seed)
    ref = K.reference(rng, length)
    samples = []
    for s in range(n_samples):
        rs = random.Random(seed * 1000 + s)
        pos = sorted(rs.randint(START - 20, START + length - 1) for _ in range(rs.randint(2, 4)))
        samples.append([K.read_for(rs, p, K.random_cigar(rs, 60), START, ref, mismatch=0.06) for p in pos])
    return (START, ref, CONTIG, samples)


def route_name(ploidy, n_samples):
    return "route p%d s%d" % (ploidy, n_samples)


def routes():
    out = []
    for ploidy, wave, block, length, seed in ROUTE_PAIRS:
        for n in (wave, block):
            out.append((route_name(ploidy, n), [route_window(seed, n, length)], K.options(ploidy)))
    return out


# ---- e. launch grids ------------------------------------------------------------------------------------------------------------

GRID_SUMS = {255: (100, 90, 65), 256: (100, 90, 66), 257: (100, 90, 67), 512: (200, 156, 1, 155)}
GRID_TAILS = (205, 206, 207)  # + max_filter_size 50 = 255, 256, 257 list entries
TAIL_OPTIONS = dict(profile_size=0, adaptive_filter_size=False, max_filter_size=50)


def grids():
    out = []
    for k, (total, lengths) in enumerate(sorted(GRID_SUMS.items())):
        windows = [K.seeded_window(540 + 10 * k + i, 1, start=1000 * (i + 1), length=n, contig=9000, max_reads=8, max_bases=80) for i, n in enumerate(lengths)]
        out.append(("%d positions in %d windows" % (total, len(lengths)), windows, K.options()))
    for n in GRID_TAILS:  # mismatches under soft clips at the window's last position: the list runs on behind it
        out.append(("%d positions and 50 list entries behind them" % n, [K.soft_clip_windows(1000, 10000, length=n, seed=560 + n)], K.options(**TAIL_OPTIONS)))
    return out


# ---- f. QUAL at both ends of `qual as u8` -----------------------------------------------------------------------------------

QUAL_AT, QUAL_DEEP_AT = 38, 30


def quals():
    """`qual as u8` saturates at both ends.  Above: ten Q40 mismatches on one position and forty on another (QUAL 320 and
    1 777), and forty matching bases on the positions around them (monomorphic with p(variant) = 0: QUAL is infinite, the
    position is not called).  Below: at the confidence threshold of every other case, 30, no QUAL is 0 -- a
    monomorphic position has QUAL = -10 log10 p(variant) with p(no variant) >= 10^-3, at least 0.0043, and any other has
    QUAL >= 30.  A threshold below 0 makes the alternate allele plausible everywhere, QUAL is -10 log10 p(no variant), and
    under eighty matching Q40 reads the posterior of the homozygous-reference genotype is 1.0 to the last bit: QUAL = 0.0."""
    ref = K.reference(random.Random(24), 60)
    deep = []
    for k in range(40):
        bases = bytearray(ref[20:45])
        bases[QUAL_DEEP_AT - 20] = other_base(bases[QUAL_DEEP_AT - 20])
        if k % 4 == 0:
            bases[QUAL_AT - 20] = other_base(bases[QUAL_AT - 20])
        deep.append((START + 20, "25M", bytes(bases), [40] * 25))
    flat = [(START + 5, "50M", ref[5:55], [40] * 50)] * 80
    return [("forty Q40 mismatches on one position", [(START, ref, CONTIG, [deep])], K.options()),
            ("eighty matching reads and a threshold below 0", [(START, ref, CONTIG, [flat])], K.options(stand_min_conf=-1.0))]


GROUPS = (("long", long), ("clips", clips), ("threshold", threshold), ("seeded", seeded), ("routes", routes), ("grids", grids), ("quals", quals))


@functools.lru_cache(maxsize=None)
def group(name):
    return dict(GROUPS)[name]()


@functools.lru_cache(maxsize=None)
def all_cases():
    return [c for g, _ in GROUPS for c in group(g)]


def case(name):
    return next(c for c in all_cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def _restated(name):
    _, windows, o = case(name)
    trace = Counter()
    return R.activity_profile(windows, trace=trace, **o), trace


def restated(name):
    """(the restatement's outputs, the quirk counters) of a case: computed once per process."""
    return _restated(name)
