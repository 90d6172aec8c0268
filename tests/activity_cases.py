"""Test infrastructure: the windows tests/test_activity_hip.py sends through phmm_activity_profile, and their restatement
(tests/activity_restatement.py), computed once per process and shared by the GPU tests and by the census of
tests/test_activity_oracle.py.  A case is (name, windows, options); a window is (start, reference bases, contig length,
per sample [(pos, cigar, bases, quals)]), which is what both lorikeet_amd.activity.pack and the restatement take."""
import functools
import random
from collections import Counter

import activity_restatement as R

BQ = 10
CONF = 30.0
PSEUDO = (10.0, 0.01, 0.00125)  # af_restatement.pseudo_counts() at the reference's defaults
BASES = b"ACGT"


def options(ploidy=2, profile_size=0, **kw):
    o = dict(ploidy=ploidy, min_base_quality=BQ, pseudo_counts=PSEUDO, stand_min_conf=CONF, max_prob_propagation=50,
             max_filter_size=50, sigma=17.0, adaptive_filter_size=True, profile_size=profile_size)
    o.update(kw)
    return o


def reference(rng, n):
    return bytes(rng.choice(BASES) for _ in range(n))


def random_cigar(rng, max_bases):
    """M / I / D / S / H / = / X in orders an aligner emits and in some it never does: clips of either quality at both ends,
    an insertion first or last, an insertion beside a deletion."""
    body, left = [], rng.randint(15, max(16, max_bases - 25))  # the insertions come on top
    lead = rng.choice([0, 0, 1, 3, 7, 12, 20])
    trail = rng.choice([0, 0, 1, 2, 6, 9, 15])
    left -= min(left - 5, lead + trail)
    if rng.random() < 0.15:
        body.append(("I", rng.randint(1, 3)))
    while left > 0:
        n = min(left, rng.randint(1, 40))
        body.append((rng.choice("MMMM=X"), n))
        left -= n
        if left > 0 and rng.random() < 0.6:
            op = rng.choice("IDD")
            body.append((op, rng.randint(1, 5)))
            if rng.random() < 0.15:
                body.append(("D" if op == "I" else "I", rng.randint(1, 3)))
    if rng.random() < 0.15:
        body.append(("I", rng.randint(1, 2)))
    cigar = ([("H", 3)] if rng.random() < 0.2 else []) + ([("S", lead)] if lead else []) + body
    cigar += ([("S", trail)] if trail else []) + ([("H", 2)] if rng.random() < 0.2 else [])
    return cigar


def read_for(rng, pos, cigar, start, ref, mismatch=0.03, low_qual=0.1):
    """Bases and qualities for a CIGAR at pos: the reference's bases with a few mismatches under M / = / X, soft clips of one
    quality class each."""
    bases, quals, at = bytearray(), [], pos
    for op, n in cigar:
        if op in "M=X":
            for k in range(n):
                b = ref[at + k - start] if 0 <= at + k - start < len(ref) else rng.choice(BASES)
                if rng.random() < mismatch:
                    b = rng.choice(bytes(set(BASES) - {b}))
                if rng.random() < 0.1:
                    b = bytes([b]).lower()[0]
                bases.append(b)
                quals.append(rng.randint(2, 9) if rng.random() < low_qual else rng.randint(10, 41))
            at += n
        elif op == "D":
            at += n
        elif op == "I":
            bases += bytes(rng.choice(BASES) for _ in range(n))
            quals += [rng.randint(2, 41) for _ in range(n)]
        elif op == "S":
            bases += bytes(rng.choice(BASES) for _ in range(n))
            q = rng.choice([5, 29, 35, 40])
            quals += [q if rng.random() < 0.9 else 28 for _ in range(n)]
    return (pos, cigar, bytes(bases), quals)


def seeded_window(seed, n_samples, start=1000, length=300, contig=100000, max_reads=64, max_bases=100):
    rng = random.Random(seed)
    ref = reference(rng, length)
    samples = []
    for s in range(n_samples):
        n = rng.randint(max_reads // 2, max_reads)
        pos = sorted(rng.randint(max(0, start - 70), start + length + 10) for _ in range(n))
        samples.append([read_for(rng, p, random_cigar(rng, max_bases), start, ref) for p in pos])
    return (start, ref, contig, samples)


SEEDED = [(1, 1, 0), (2, 1, 128), (2, 2, 0), (3, 2, 128), (1, 4, 128), (3, 4, 0), (1, 64, 0), (2, 64, 128)]  # samples, ploidy, profile size


def seeded():
    return [("seeded s%d p%d c%d" % c, [seeded_window(100 + i, c[0])], options(c[1], c[2])) for i, c in enumerate(SEEDED)]


def one_read(name, pos, cigar, ref, start=500, contig=50000, bases=None, quals=None, seed=7, **kw):
    """A window with one read; `bases` / `quals` default to the reference's bases at Q30."""
    rng = random.Random(seed)
    if bases is None:
        _, _, bases, quals0 = read_for(rng, pos, R.parse_cigar(cigar), start, ref, mismatch=0.0, low_qual=0.0)
        bases = bases.upper()
        quals = quals if quals is not None else [30] * len(quals0)
    return (name, [(start, ref, contig, [[(pos, cigar, bases, quals)]])], options(**kw))


def quirks():
    rng = random.Random(11)
    ref = reference(rng, 60)
    S, E = 500, 560
    mism = lambda b: bytes([BASES[(BASES.index(bytes([b]).upper()) + 1) % 4]])[0]  # noqa: E731
    out = []
    # an I element: one entry at the current position, its first base against the reference base there -- equal and different
    for tag, first in (("matches", ref[20]), ("differs", mism(ref[20]))):
        bases = ref[10:20] + bytes([first]) + b"T" + ref[20:30]
        out.append(one_read("insertion whose first base %s" % tag, S + 10, "10M2I10M", ref, bases=bases, quals=[30] * 22))
    # an I element before bound_start: cig_index lags, and the deletion's neighbours are read one element early
    out.append(one_read("lagging cig_index hides the soft clip", S - 10, "5M2I10M3D4S", ref))
    out.append(one_read("lagging cig_index finds a soft clip", S - 1, "2I4S1M3D10M", ref))
    out.append(one_read("no lag: the same deletion inside the window", S + 2, "5M2I10M3D4S", ref))
    # past bound_end: an I element ends the read, a D / M element itself
    out.append(one_read("insertion at bound_end", E - 10, "10M2I5M", ref))
    out.append(one_read("insertion past bound_end", E - 10, "20M2I20M", ref))
    out.append(one_read("deletion over bound_end", E - 8, "5M20D5M", ref))
    out.append(one_read("match over bound_end then soft clip", E - 8, "30M5S", ref))
    # next_to_soft_clip_or_indel: leading and trailing clips, clips of one base, an insertion at the very start, I beside D
    for cg in ("6S20M", "20M7S", "1S20M1S", "3H8S10M2D10M9S2H", "2I20M", "20M2I", "10M2I3D10M", "10M3D2I10M", "5M1I1M1D5M", "8S1M8S", "10=5X10="):
        out.append(one_read("adjacency %s" % cg, S + 5, cg, ref, quals=None))
    # is_alt is never evaluated for an uncounted base: a low-quality mismatch beside a soft clip adds no soft clips
    bases = b"A" * 8 + bytes([mism(ref[5])]) + ref[6:25]
    out.append(one_read("uncounted mismatch beside a clip", S + 5, "8S20M", ref, bases=bases, quals=[40] * 8 + [3] + [30] * 19))
    out.append(one_read("counted mismatch beside a clip", S + 5, "8S20M", ref, bases=bases, quals=[40] * 8 + [30] * 20))
    out.append(one_read("lower-case bases", S + 5, "20M", ref.lower(), bases=ref[5:25].upper(), quals=[30] * 20))
    return out


def panics():
    """N in a CIGAR and CIGARs that consume more bases than the read has, between intact neighbours."""
    good = [seeded_window(40, 2, start=2000, length=60, max_reads=6, max_bases=40), seeded_window(41, 2, start=9000, length=50, max_reads=6, max_bases=40)]
    rng = random.Random(5)
    ref = reference(rng, 40)
    n_win = (700, ref, 5000, [[(705, "10M", ref[5:15], [30] * 10)], [(700, "5M3N5M", ref[0:5] + ref[8:13], [30] * 10)]])
    over = (700, ref, 5000, [[(702, "10M2S", ref[2:12] + b"A", [30] * 11)], []])
    over_i = (700, ref, 5000, [[], [(702, "10M5I", ref[2:12] + b"ACG", [30] * 13)]])
    return [("panics", [good[0], n_win, over, good[1], over_i], options())]


def soft_clip_windows(start, contig, length=120, seed=3, n_reads=5, clip=14):
    """Reads whose clips put the running average above 6 at both ends of the window and a mismatch in every read."""
    rng = random.Random(seed)
    ref = reference(rng, length)
    reads = []
    for k in range(n_reads):
        reads.append((start, [("S", clip), ("M", 30)], b"G" * clip + bytes([BASES[(BASES.index(ref[0:1]) + 1) % 4]]) + ref[1:30], [35] * (clip + 30)))
    mid = start + length // 2
    reads.append((mid, "25M", ref[length // 2:length // 2 + 12] + b"N" + ref[length // 2 + 13:length // 2 + 25], [33] * 25))
    for k in range(n_reads):
        p = start + length - 30
        reads.append((p, [("M", 30), ("S", clip)], ref[length - 30:length - 1] + bytes([BASES[(BASES.index(ref[-1:]) + 1) % 4]]) + b"C" * clip, [35] * (clip + 30)))
    return (start, ref, contig, [reads])


def edges():
    out = [("window at position 0", [soft_clip_windows(0, 10000)], options()),
           ("window below F", [soft_clip_windows(20, 10000, seed=4)], options(profile_size=50)),
           ("window ending within F of the contig", [soft_clip_windows(880, 1010, seed=5)], options()),
           ("window ending at the contig's last base", [soft_clip_windows(880, 1000, seed=6)], options(profile_size=64)),
           ("window ending one before the contig's last base", [soft_clip_windows(880, 1001, seed=8)], options()),
           ("fixed filter size and a short propagation", [soft_clip_windows(30, 400, seed=9)],
            options(adaptive_filter_size=False, max_filter_size=12, sigma=3.0, max_prob_propagation=9)),
           ("an empty window and a sample without reads",
            [(300, b"", 5000, [[], []]), (400, reference(random.Random(2), 30), 5000, [[], [(405, "10M", b"ACGTACGTAC", [30] * 10)]]),
             (100, reference(random.Random(3), 10), 5000, [[], []])], options())]
    return out


def large():
    """One window of 20 000 positions under 2 000 reads beside 63 small ones: workgroup and wave boundaries, the read-range
    index and the workspace offsets are crossed.  The large window starts past 2^33."""
    big = seeded_window(77, 1, start=(1 << 33) + 5, length=20000, contig=1 << 34, max_reads=2000, max_bases=100)
    rng = random.Random(78)
    small = [seeded_window(200 + i, 1, start=rng.randint(0, 3000), length=rng.randint(1, 70), contig=4000, max_reads=4, max_bases=40) for i in range(63)]
    return [("large", small[:30] + [big] + small[30:], options(ploidy=2, profile_size=0))]


@functools.lru_cache(maxsize=None)
def all_cases():
    return seeded() + quirks() + panics() + edges() + large()


@functools.lru_cache(maxsize=None)
def _restated(name):
    for n, windows, o in all_cases():
        if n == name:
            trace = Counter()
            return R.activity_profile(windows, trace=trace, **o), trace
    raise KeyError(name)


def restated(name):
    """(the restatement's outputs, the quirk counters) of a case: computed once per process."""
    return _restated(name)
