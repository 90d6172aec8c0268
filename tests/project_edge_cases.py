"""Inputs of phmm_project_to_reference that the aligner never emits (tests/test_project_edge_table.py holds them against the
oracle alone, tests/test_project_edges_hip.py holds the device against the oracle on them): read -> haplotype alignments
written by hand or drawn at random over all nine operators, with zero-length elements, deletions at the ends and next to
insertions, indels at the right end of repeats, reads on both sides of the `plain` short cut's condition, and batches on both
sides of the line between the lanes' builders in LDS and in HBM.  Plain numpy, no GPU.

Every builder returns what realign.project_to_reference takes -- (batch, best alleles, alignments, haplotype CIGARs, haplotype
starts, reference haplotype per region, reference start per region, original CIGARs) -- and is a function of its arguments
alone (the generators are seeded with crc32(repr(key)))."""
import functools
import re
import zlib

import numpy as np

from lorikeet_amd.batch import RegionBatch
from lorikeet_amd.smith_waterman import SmithWatermanAlignmentResult
from oracle import oracle
from oracle.oracle import CigarError

OPS = "MIDNSHP=X"
ON_READ = "MIS=X"
ALPHA = b"ACGT"

# the constants of lorikeet_amd/csrc the batches are shaped by (tests/test_project_edge_table.py reads them out of the sources)
PLAIN_PAD = 1000            # get_consolidated_padded_cigar(1000): the short cut holds up to offset + read length == h + 1000
LDS_MAX_READS = 4096        # launch_project / launch_pick: a larger launch keeps the builders in HBM
LDS_BLOCK, HBM_BLOCK = 32, 64
LDS_BYTES = 64 * 1024
FUSED_SW_SLOTS = 24         # alignment elements phmm_realign_reads reserves per read on the device


def capacity(max_sw, max_hc):
    """Elements per builder as the host derives them (phmm_cigar.cpp)."""
    return 4 * (max_sw + max_hc + 2) + 8


def lds_bytes(n_elements):
    """Dynamic LDS of a launch whose longest alignment and longest haplotype CIGAR have n_elements together."""
    return LDS_BLOCK * 4 * capacity(n_elements, 0) * 4


LAST_LDS_N = max(n for n in range(200) if lds_bytes(n) <= LDS_BYTES)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _rnd(rng, n, k=4):
    return bytes(ALPHA[int(x)] for x in rng.integers(0, k, n))


def elements(text):
    """'3M2D' -> [(3, 'M'), (2, 'D')]."""
    return [(int(n), o) for n, o in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def read_len(text):
    return sum(n for n, o in elements(text) if o in ON_READ)


class _Regions:
    """Regions under construction: haplotypes (the reference haplotype first) and reads with their hand-made alignments."""

    def __init__(self):
        self.regions = []

    def region(self, haps, hap_cigars, hap_starts, ref_start):
        assert len(haps) == len(hap_cigars) == len(hap_starts) and len(haps) >= 1
        self.regions.append(dict(haps=list(haps), cigars=list(hap_cigars), starts=list(hap_starts), ref_start=int(ref_start), reads=[]))
        return len(self.regions) - 1

    def read(self, g, bases, best, alignment, offset, original):
        """alignment: CIGAR text (None: the read has no alignment), offset: its alignment_offset."""
        self.regions[g]["reads"].append((bytes(bases), int(best), alignment, int(offset), original))

    def inputs(self):
        rro, rho, ro, ho, oo = [0], [0], [0], [0], [0]
        rb, hb, best, aligned, hap_cigars, hap_starts, ref_hap, ref_start, orig = [], [], [], [], [], [], [], [], []
        for reg in self.regions:
            for bases, k, aln, off, original in reg["reads"]:
                assert -1 <= k < len(reg["haps"])
                rb.append(bases)
                ro.append(ro[-1] + len(bases))
                best.append(k)
                aligned.append(None if aln is None else SmithWatermanAlignmentResult(oracle.parse_cigar(aln), off))
                orig.append(oracle.parse_cigar(original))
            for h, c, s in zip(reg["haps"], reg["cigars"], reg["starts"]):
                hb.append(bytes(h))
                ho.append(ho[-1] + len(h))
                hap_cigars.append(oracle.parse_cigar(c))
                hap_starts.append(int(s))
            rro.append(rro[-1] + len(reg["reads"]))
            rho.append(rho[-1] + len(reg["haps"]))
            oo.append(oo[-1] + len(reg["reads"]) * len(reg["haps"]))
            ref_hap.append(0)
            ref_start.append(reg["ref_start"])
        read_bases = np.frombuffer(b"".join(rb), np.uint8).copy()
        n = len(read_bases)
        b = RegionBatch(region_read_off=np.asarray(rro, np.uint32), region_hap_off=np.asarray(rho, np.uint32), read_off=np.asarray(ro, np.uint32),
                        hap_off=np.asarray(ho, np.uint32), out_off=np.asarray(oo, np.uint64), read_bases=read_bases,
                        base_q=np.full(n, 30, np.uint8), ins_q=np.full(n, 45, np.uint8), del_q=np.full(n, 45, np.uint8),
                        gcp=np.full(n, 10, np.uint8), hap_bases=np.frombuffer(b"".join(hb), np.uint8).copy())
        return b, np.asarray(best, np.int32), aligned, hap_cigars, hap_starts, ref_hap, ref_start, orig


def read_region(inputs):
    b = inputs[0]
    return np.repeat(np.arange(b.n_regions), np.diff(b.region_read_off.astype(np.int64)))


def oracle_read(inputs, r, g):
    """(status, pos, cigar string) of the oracle for read r of region g FROM THE GIVEN ALIGNMENT."""
    b, best, aligned, hap_cigars, hap_starts, ref_hap, ref_start, orig = inputs
    if best[r] < 0 or aligned[r] is None:
        return 1, 0, ""
    hp = int(b.region_hap_off[g]) + int(best[r])
    hr = int(b.region_hap_off[g]) + ref_hap[g]
    ref = b.hap_bases[int(b.hap_off[hr]):int(b.hap_off[hr + 1])]
    read = b.read_bases[int(b.read_off[r]):int(b.read_off[r + 1])]
    try:
        res = oracle.create_read_aligned_to_ref(aligned[r].elements, aligned[r].alignment_offset, hap_cigars[hp], hap_starts[hp], ref_start[g],
                                                ref, read, orig[r])
    except CigarError as e:
        return e.code, 0, ""
    return (1, 0, "") if res is None else (0, int(res[0]), res[1])


def oracle_all(inputs):
    reg = read_region(inputs)
    return [oracle_read(inputs, r, int(reg[r])) for r in range(inputs[0].n_reads)]


def describe(inputs, r):
    """The read's inputs as text, for failure messages."""
    b, best, aligned, hap_cigars, hap_starts, ref_hap, ref_start, orig = inputs
    g = int(read_region(inputs)[r])
    hp = int(b.region_hap_off[g]) + max(int(best[r]), 0)
    aln = "none" if aligned[r] is None else "%s @ %d" % (oracle.cigar_to_string(aligned[r].elements), aligned[r].alignment_offset)
    return "read %d (%d bases, region %d): alignment %s, haplotype %d %s start %d, original %s" % (
        r, int(b.read_off[r + 1]) - int(b.read_off[r]), g, aln, int(best[r]), oracle.cigar_to_string(hap_cigars[hp]) if best[r] >= 0 else "-",
        hap_starts[hp] if best[r] >= 0 else 0, oracle.cigar_to_string(orig[r]))


def histogram(expected):
    h = {}
    for st, _, _ in expected:
        h[st] = h.get(st, 0) + 1
    return dict(sorted(h.items()))


def originals(n):
    """The original CIGARs of builder b for a read of n bases."""
    return ["%dM" % n, "3H2S%dM1S" % n, "2S%dM4H" % n, "5S", "2H"]


# ---- a: the operator-pair table ---------------------------------------------------------------------------------------
TABLE_CASES = [(flank, letters) for flank in "M=X" for letters in (4, 2)]
TABLE_OFFSETS = range(9)


def table_rows(a, c, flank):
    """(alignment, haplotype CIGAR) of the pair (a, c): `4M 3a 4M` against `6M 5c 200M`.  An S between two aligned blocks is
    the builder's order error in the reference ("Cigar has already reached its right (hard) clip"), on either side -- so a pair
    with an S also gets the S at the end where it is legal: `3S 8M`, `8M 3S`, and the haplotype `5S 206M`."""
    f = flank
    rows = [("4%s3%s4%s" % (f, a, f), "6%s5%s200%s" % (f, c, f))]
    if a == "S" or c == "S":
        alns = ["3S8%s" % f, "8%s3S" % f] if a == "S" else [rows[0][0]]
        hcs = ["5S206%s" % f] if c == "S" else [rows[0][1]]
        rows += [(x, y) for x in alns for y in hcs]
    return rows


@functools.lru_cache(maxsize=None)
def table(flank, letters):
    """-> (inputs, {(a, c): [read indices]})."""
    rng = _rng("table", flank, letters)
    R = _Regions()
    reference = _rnd(rng, 240, letters)
    where, at = {}, 0
    for a in OPS:
        hap_cigars, index = ["240M"], {}
        for c in OPS:
            for _, hc in table_rows(a, c, flank):
                if hc not in index:
                    index[hc] = len(hap_cigars)
                    hap_cigars.append(hc)
        haps = [reference] + [(reference + reference)[:max(1, read_len(hc))] for hc in hap_cigars[1:]]
        g = R.region(haps, hap_cigars, [0] + [int(x) for x in rng.integers(0, 3, len(haps) - 1)], rng.integers(1, 10 ** 9))
        for c in OPS:
            for aln, hc in table_rows(a, c, flank):
                n = read_len(aln)
                for off in TABLE_OFFSETS:
                    bases = bytearray(reference[off:off + n])
                    if n and rng.random() < 0.3:
                        bases[int(rng.integers(0, n))] = ALPHA[int(rng.integers(0, letters))]
                    R.read(g, bases, index[hc], aln, off, originals(n)[(off + at) % 3])
                    where.setdefault((a, c), []).append(at)
                    at += 1
    return R.inputs(), where


# ---- b: the builder's rules on the alignment side -------------------------------------------------------------------
RULE_ALIGNMENTS = [
    "3D5M", "2I3D5M", "2S3D5M", "2H2S3D5M",                                            # a deletion before anything aligned
    "5M3D", "5M3D2I", "5M3D2S", "5M3D2I2S", "5M2I3D4M", "5M3D2I3D4M", "5M0D4M", "0M5M",  # ... at the end, beside an insertion, zero lengths
    "5M2S3M", "5M2H2S", "5S", "3D", "2I", "3D2I", "5M3N4M", "5M2P4M",                   # the builder's errors; operators without a transform
    "2H5M", "5M2H", "2S5M2S", "5M2I3D", "5M2D3D4M", "0D5M0I", "5M2S2S", "5M3D2H", "2I5M", "5M2I", "3D2I5M", "5M3D0S",
]
RULE_OFFSETS = (0, 17)


@functools.lru_cache(maxsize=None)
def rules(letters):
    rng = _rng("rules", letters)
    R = _Regions()
    reference = _rnd(rng, 120, letters)
    hap_cigars = ["120M", "20M2D98M", "20M2I100M"]
    haps = [reference, reference[:20] + reference[22:], reference[:20] + _rnd(rng, 2, letters) + reference[20:]]
    g = R.region(haps, hap_cigars, [0, 2, 1], rng.integers(1, 10 ** 9))
    for aln in RULE_ALIGNMENTS:
        n = read_len(aln)
        for k in range(3):
            for off in RULE_OFFSETS:
                for original in originals(n):
                    R.read(g, haps[k][off:off + n], k, aln, off, original)
    return R.inputs()


# ---- c: left_align_indels -----------------------------------------------------------------------------------------------
UNITS = {1: b"A", 2: b"AC", 3: b"ACG"}
REPEATS = 6


def _flank(rng, n):
    """n letters of G / T (the units have none), so that the repeat neither starts earlier nor ends later than it is written."""
    return bytes(b"GT"[int(x)] for x in rng.integers(0, 2, n))


def _repeat_reads(hap, rep_start, rep_end, u, s, e, rng):
    """Reads cut out of hap[s:e] with one or two units of the repeat hap[rep_start:rep_end] inserted or deleted, the indel
    written at the RIGHTMOST equivalent position; two indels in one repeat closer than the repeat can shift; an indel behind
    an S or an I.  -> [(bases, alignment)]"""
    unit = hap[rep_start:rep_start + u]
    left, right = rep_end - s, e - rep_end            # bases of the read up to the repeat's end, and behind it
    out = []
    tail = ("%dM" % right) if right > 0 else ""
    for m in (1, 2):
        d = m * u
        if left - d > 0:
            out.append((hap[s:rep_end - d] + hap[rep_end:e], "%dM%dD%s" % (left - d, d, tail)))
        out.append((hap[s:rep_end] + unit * m + hap[rep_end:e], "%dM%dI%s" % (left, d, tail)))
    if left - 3 * u > 0:   # two indels, one unit of matches between them
        a = left - 3 * u
        out.append((hap[s:rep_end - 2 * u] + hap[rep_end:e], "%dM%dD%dM%dD%s" % (a, u, u, u, tail)))                       # -1 -1
        out.append((hap[s:rep_end] + unit * 2 + hap[rep_end:e], "%dM%dI%dM%dI%s" % (left - u, u, u, u, tail)))              # +1 +1
        out.append((hap[s:e], "%dM%dI%dM%dD%s" % (left - 2 * u, u, u, u, tail)))                                              # +1 -1
        out.append((hap[s:e], "%dM%dD%dM%dI%s" % (a, u, 2 * u, u, tail)))                                                     # -1 +1
    junk = _rnd(rng, 3)
    if left - u > 0:       # the indel's left neighbour is a clip or an insertion
        out.append((junk + hap[s + u:e], "3S%dD%s" % (u, "%dM" % (e - s - u))))
        out.append((junk + unit + hap[s:e], "3S%dI%dM" % (u, e - s)))
        out.append((hap[s:rep_end - u] + junk[:2] + hap[rep_end:e], "%dM2I%dD%s" % (left - u, u, tail)))
        out.append((junk[:2] + hap[s + u:e], "2I%dD%dM" % (u, e - s - u)))
    return out


@functools.lru_cache(maxsize=None)
def repeats(u):
    """Repeat unit of u letters; one region per distance d of the repeat from the read's first base and alignment offset
    (0: the read starts at the haplotype's first base; > 0)."""
    R = _Regions()
    unit = UNITS[u]
    for d in list(range(0, u + 3)) + [-u]:
        for lead in (0, 9):                   # alignment_offset of the reads
            for right in (14, 0):             # unique bases behind the repeat; 0: the repeat runs to the reference's last base
                rng = _rng("repeats", u, d, lead, right)
                left = lead + max(d, 0)
                reference = _flank(rng, left) + unit * REPEATS + _flank(rng, right)
                rs, re_ = left, left + u * REPEATS
                # the haplotypes: the reference twice (start 0 and > 0), and two that carry their own indel inside the repeat
                at = rs + 2 * u
                hap_d = reference[:at] + reference[at + u:]
                hap_i = reference[:at] + unit + reference[at:]
                n = len(reference)
                haps = [reference, reference, hap_d, hap_i]
                cigars = ["%dM" % n, "%dM" % n, "%dM%dD%dM" % (at, u, n - at - u), "%dM%dI%dM" % (at, u, n - at)]
                g = R.region(haps, cigars, [0, 7, 0, 3], rng.integers(1, 10 ** 9))
                s = lead if d >= 0 else rs + u
                for k, hap in enumerate(haps):
                    h_re = re_ + (len(hap) - n)   # the repeat's end on this haplotype
                    ends = {min(h_re + 8, len(hap)), len(hap)}
                    for e in sorted(ends):
                        for bases, aln in _repeat_reads(hap, rs, h_re, u, s, e, rng):
                            R.read(g, bases, k, aln, s, "%dM" % len(bases) if (e + k) % 2 else "2S%dM3H" % len(bases))
                    # one base past the haplotype's end ("Read goes past end of reference" where an indel stands there)
                    e = len(hap)
                    extra = _rnd(rng, 1)
                    R.read(g, hap[s:e] + extra + unit, k, "%dM%dI" % (e - s + 1, u), s, "%dM" % (e - s + 1 + u))
                    R.read(g, hap[s:e] + unit, k, "%dM%dI" % (e - s, u), s, "%dM" % (e - s + u))
                    R.read(g, hap[s:e - u] + extra, k, "%dM%dD1M" % (e - s - u, u), s, "%dM" % (e - s - u + 1))
    return R.inputs()


# ---- d: the `plain` short cut's boundary --------------------------------------------------------------------------------
PLAIN_DELTAS = (999, 1000, 1001)
PLAIN_SPELLINGS = ("plain", "insertion", "equal")


def plain_spelling(kind, n):
    return {"plain": "%dM" % n, "insertion": "%dM1I" % (n - 1), "equal": "1=%dM" % (n - 1)}[kind]


@functools.lru_cache(maxsize=None)
def plain():
    """-> (inputs, rows): rows = [(read index, spelling, delta, longer)] for the reads at the boundary; `longer` is how many
    bases the read has more than its alignment (0, +1, -1: the reference's length check; one base behind the line the haplotype's
    padded CIGAR ends one base early, and it is the read with one base less that passes).
    The reference haplotype is long enough for the reads to lie on it at offsets around 1000 -- the non-plain spellings go
    through left_align_indels, which refuses a read behind the reference's end."""
    rng = _rng("plain")
    R = _Regions()
    rows, at = [], 0
    reference = _rnd(rng, 1000 + 320 + 130)
    for h in (1, 40, 300):
        g = R.region([reference, reference[:h], reference[:h]], ["%dM" % len(reference), "%dM" % h, "%dM" % h], [0, 0, 4], rng.integers(1, 10 ** 9))
        for n in (2, 3, 50, 120):
            for delta in PLAIN_DELTAS + (0,):
                off = delta + h - n
                if off < 0:
                    continue
                for kind in PLAIN_SPELLINGS:
                    for longer in (0, 1, -1):
                        R.read(g, reference[off:off + n + longer], 1 + (n + delta) % 2, plain_spelling(kind, n), off, "%dM" % (n + longer))
                        if delta in PLAIN_DELTAS:
                            rows.append((at, kind, delta, longer))
                        at += 1
        # no bases at all, and offsets below 0
        for aln in ("0M", "5M", ""):
            for off in (0, -1, -2):
                R.read(g, b"", 1, aln, off, "5S")
                at += 1
        for off in (-1, -2, 0):
            R.read(g, reference[:30], 1, "30M", off, "30M")
            R.read(g, reference[:30], 1, "29M1I", off, "2S30M")
            at += 2
    return R.inputs(), rows


# ---- e: random hand-built alignments ------------------------------------------------------------------------------------
RANDOM_CLASSES = [("MID", "MID"), ("MIDS", "MID"), ("MID=X", "MIDS=X"), (OPS, OPS)]
RANDOM_READS = 1700


def _random_cigar(rng, ops, n_max, len_max, weight_m):
    n = int(rng.integers(1, n_max + 1))
    p = np.array([weight_m if o == "M" else 1.0 for o in ops])
    out = []
    for o in rng.choice(list(ops), n, p=p / p.sum()):
        out.append("%d%s" % (0 if rng.random() < 0.05 else int(rng.integers(1, len_max + 1)), o))
    return "".join(out)


def _random_region(R, rng, cls, n_reads, short=False):
    aln_ops, hap_ops = RANDOM_CLASSES[cls]
    letters = 2 if rng.random() < 0.3 else 4
    reference = _rnd(rng, int(rng.integers(60, 120) if short else rng.integers(150, 320)), letters)
    haps, cigars = [reference], ["%dM" % len(reference)]
    for _ in range(int(rng.integers(1, 4))):
        hc = _random_cigar(rng, hap_ops, 3 if short else 5, 30 if short else 80, 4.0)
        cigars.append(hc)
        haps.append((reference + reference + reference)[:max(1, min(read_len(hc), 320))])
    g = R.region(haps, cigars, [0] + [int(x) for x in rng.integers(0, 4, len(haps) - 1)], rng.integers(1, 10 ** 9))
    for _ in range(n_reads):
        k = int(rng.integers(0, len(haps)))
        aln = _random_cigar(rng, aln_ops, 3 if short else 6, 6 if short else 20, 3.0)
        if aln_ops == OPS and rng.random() < 0.5:   # clips where they are legal, too
            aln = ("%dS" % rng.integers(1, 4) if rng.random() < 0.5 else "") + aln + ("%dS" % rng.integers(1, 4) if rng.random() < 0.5 else "")
        n = read_len(aln)
        if rng.random() < 0.15:
            n = max(0, n + int(rng.integers(-2, 3)))
        u = rng.random()
        off = int(rng.integers(0, 30)) if u < 0.9 else (-1, -1, -2, 2000)[int(rng.integers(0, 4))]
        if rng.random() < 0.6:
            s = max(0, min(off, len(reference)))
            bases = (reference[s:] + reference)[:n]
        else:
            bases = _rnd(rng, n, letters)
        R.read(g, bases, k, aln, off, originals(n)[int(rng.integers(0, 5))])


def _random_regions(cls, n_reads):
    rng = _rng("random", cls)
    R = _Regions()
    left = n_reads
    while left:
        n = min(left, int(rng.integers(5, 40)))
        _random_region(R, rng, cls, n)
        left -= n
    return R


@functools.lru_cache(maxsize=None)
def random_alignments(cls, n_reads=RANDOM_READS):
    return _random_regions(cls, n_reads).inputs()


# ---- f: the workspace boundary ---------------------------------------------------------------------------------------------
def long_alignment(rng, reference, s, n_elements):
    """A legal alignment of exactly n_elements: 3M and one-base indels in turn (behind a 2S where the count is even), the read
    made from reference[s:] to fit -> (bases, alignment)."""
    bases, aln, at = bytearray(), [], s
    if n_elements % 2 == 0:
        bases += _rnd(rng, 2)
        aln.append("2S")
    k = 0
    while len(aln) < n_elements:
        if k % 2 == 0:
            bases += reference[at:at + 3]
            at += 3
            aln.append("3M")
        elif k % 4 == 1:
            bases += _rnd(rng, 1)
            aln.append("1I")
        else:
            at += 1
            aln.append("1D")
        k += 1
    assert at <= len(reference) and len(elements("".join(aln))) == n_elements
    return bytes(bases), "".join(aln)


WORKSPACE_BASE = (2, 400)       # the random batch (class, reads) the long alignment stands beside


@functools.lru_cache(maxsize=None)
def workspace(n_total):
    """The random batch e (class MID=X / MIDS=X, 400 reads) and one more region whose single read carries an alignment of
    n_total - max_hc elements -> (inputs, index of the long read, its element count)."""
    cls, n = WORKSPACE_BASE
    R = _random_regions(cls, n)       # random_alignments(cls, n): the reads common to every n_total
    max_hc = max(len(elements(c)) for reg in R.regions for c in reg["cigars"])
    pad = n_total - max_hc
    rng = _rng("workspace")
    reference = _rnd(rng, 200)
    bases, aln = long_alignment(rng, reference, 11, pad)
    g = R.region([reference, reference[:60] + reference[62:]], ["200M", "60M2D138M"], [0, 1], 12345)
    R.read(g, bases, 0, aln, 11, "1S%dM2H" % len(bases))
    return R.inputs(), n, pad


COUNT_CASES = [(n, LAST_LDS_N) for n in (1, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097)] + [(n, LAST_LDS_N + 1) for n in (4095, 4096, 4097)]
COUNT_MAX_HC = 3


@functools.lru_cache(maxsize=None)
def _count_regions(n_total):
    """4 097 reads: the long read (n_total - 3 elements) first, then short ones (<= 3 elements against <= 3) in regions of 40."""
    R = _Regions()
    rng = _rng("count")
    reference = _rnd(rng, 200)
    bases, aln = long_alignment(_rng("count long", n_total), reference, 5, n_total - COUNT_MAX_HC)
    g = R.region([reference, reference[:50] + reference[51:] + b"A"], ["200M", "50M1D%dM" % 150], [0, 2], 777)
    R.read(g, bases, 0, aln, 5, "%dM" % len(bases))
    for _ in range(39):
        s = int(rng.integers(0, 150))
        R.read(g, reference[s:s + 12], 1, "12M" if rng.random() < 0.5 else "5M1D6M1I", s, "12M")
    for _i in range(102):
        _random_region(R, rng, 0, 40, short=True)
    return R


@functools.lru_cache(maxsize=None)
def count(n_reads, n_total):
    """The first n_reads reads of the same 4 120: whole regions and the beginning of the next."""
    full = _count_regions(n_total)
    R = _Regions()
    left = n_reads
    for reg in full.regions:
        if not left:
            break
        R.regions.append(dict(reg, reads=reg["reads"][:left]))
        left -= len(R.regions[-1]["reads"])
    assert not left
    return R.inputs()


def host_max(inputs):
    """(max_sw, max_hc) as phmm_project_to_reference computes them."""
    return max((len(a.elements) for a in inputs[2] if a is not None), default=0), max(len(c) for c in inputs[3])
