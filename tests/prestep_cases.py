"""Inputs that reach the whole of the pre-step (prepdev::prep_read_wave and tandem_repeat_length, lorikeet_amd/csrc/
phmm_prep_device.hpp), and a plain restatement of it with switches for deliberately wrong variants.  tests/test_prestep_table.py
holds both to the oracle alone and proves that every wrong variant would show; tests/test_prestep_hip.py runs the inputs through
every route that launches the pre-step.  numpy and the oracle only: no GPU needed to import it.

The pre-step has no output of its own: it shows through the likelihoods (insertion / deletion / base qualities) and the keep
flags (the threshold).  The PCR caches are coarse -- repeat lengths 1 and 2 share a value under every model, every length above
33 gives 6 -- so the reads are built around STR alleles at lengths the caches resolve (3, 4 and 6 copies of units of 1 ... 20
bases), and the mutants below are the proof that a wrong scan moves a likelihood by a thousand tolerances.

Mutants of the scan and the qualities (wrong on the CPU only):
  a        a unit length is accepted on the screen alone (the first two positions recur at that distance)
  b        the search stops at the first screen candidate, also where the exact test rejects it
  c19 c16  unit lengths stop at 19 / at 16
  d_before d_past   positions before the read's start / past its end compare equal (a copy that is partly outside counts)
  e_start  e_end    a copy that starts exactly at 0 / ends exactly at n is not accepted
  f_add    backward and forward counts are added as if the units were equal
  f_norecount       a forward unit that differs from the backward unit is not counted again behind the offset
  g_last   the last base gets the model too;  g_skip: offset n - 2 skips the forward scan
  h        positions from 64 on keep their input qualities (a stride loop that runs once)
  i        min(tag, cache) always takes the cache
Mutants of the threshold:
  j_floor j_round   ceil becomes floor / round to nearest
  k_minus k_plus    the table index is one off
  l        the threshold is computed from the modified base qualities
  m        min(dyn, cap) becomes max"""
import functools
import math
import zlib
from collections import namedtuple

import numpy as np

from lorikeet_amd.batch import Read, RegionBatch
from oracle import oracle
from project_scenarios import ALPHA, rnd
from server_instance_cases import SRV_MAX_ROWS, _assemble
from test_region_hip import MODELS, _oracle_pipeline

MAX_STR_UNIT_LENGTH, MAX_REPEAT_LENGTH, MIN_USABLE_Q, DEFAULT_INDEL_Q = 20, 100, 6, 45
SCAN_MUTANTS = ("a", "b", "c19", "c16", "d_before", "d_past", "e_start", "e_end", "f_add", "f_norecount", "g_last", "g_skip")
QUALITY_MUTANTS = SCAN_MUTANTS + ("h", "i")
THRESHOLD_MUTANTS = ("j_floor", "j_round", "k_minus", "k_plus", "l", "m")


# ---- the scan, restated: find_tandem_repeat_units as the reference's nested loops ---------------------------------------------
def _count(s, u, ln, lo, tl, leading, partial=False):
    """find_number_of_repetitions_main on one string: copies of s[u:u+ln] in s[lo:lo+tl], from the front or from the back.
    partial (mutants d): one more copy, partly outside the string, counts where its inside part matches."""
    if tl == 0:
        return 0
    unit, diff, c = s[u:u + ln], tl - ln, 0
    if leading:
        st = 0
        while st <= diff:
            if s[lo + st:lo + st + ln] != unit:
                return c
            c += 1
            st += ln
        if partial and st < tl and s[lo + st:lo + tl] == unit[:tl - st]:
            c += 1
        return c
    st = diff
    while st >= 0:
        if s[lo + st:lo + st + ln] != unit:
            return c
        c += 1
        st -= ln
    if partial and st + ln > 0 and s[lo:lo + st + ln] == unit[-(st + ln):]:
        c += 1
    return c


Scan = namedtuple("Scan", "length uncapped bw_len fw_len bw_rejected fw_rejected")


def scan(s, offset, mutant=None):
    """Scan.length: the repeat length the pre-step looks up for position `offset` of read s (bytes).  bw_len / fw_len: the unit
    length the backward / forward search accepted (0: none); *_rejected: the longest length BELOW the accepted one at which
    the first two positions recurred (the device's screen) while the unit did not."""
    n = len(s)
    longest = {"c19": 19, "c16": 16}.get(mutant, MAX_STR_UNIT_LENGTH)

    # (find_number_of_repetitions_main gives 1 -- the unit itself -- unless the copy next to the unit equals it: the count is
    # asked for only there, and under the mutants d, whose copies may lie partly outside the read)
    count_all = mutant in ("d_before", "d_past")
    max_bw, bw_u, bw_len, bw_hit, bw_rej = 0, offset, 1, 0, 0
    for k in range(1, longest + 1):
        if offset + 1 < k:
            break
        a = offset + 1 - k
        max_bw = _count(s, a, k, 0, offset + 1, False, mutant == "d_before") if count_all or (a >= k and s[a - k:a] == s[a:a + k]) else 1
        ok = max_bw > 1
        if mutant == "e_start" and a - k == 0:
            ok, max_bw = False, 1
        if ok:
            bw_u, bw_len, bw_hit = a, k, k
            break
        # the device's screen: the first two positions recur k bases earlier (positions outside the read never compare equal)
        if a >= 1 and s[offset] == s[a - 1] and (k < 2 or (a >= 2 and s[offset - 1] == s[a - 2])):
            if mutant == "a":
                bw_u, bw_len, bw_hit = a, k, k
                break
            bw_rej = k
            if mutant == "b":
                break
    max_rl, fw_hit, fw_rej = max_bw, 0, 0
    if offset < n - 1 and not (mutant == "g_skip" and offset == n - 2):
        max_fw, fw_u, fw_len = 0, offset + 1, 1
        for k in range(1, longest + 1):
            if offset + k + 1 > n:
                break
            a = offset + 1
            max_fw = (_count(s, a, k, a, n - a, True, mutant == "d_past") if count_all or (a + 2 * k <= n and s[a + k:a + 2 * k] == s[a:a + k])
                      else 1)
            ok = max_fw > 1
            if mutant == "e_end" and a + 2 * k == n:
                ok, max_fw = False, 1
            if ok:
                fw_len, fw_hit = k, k
                break
            if a + k < n and s[a] == s[a + k] and (k < 2 or (a + 1 + k < n and s[a + 1] == s[a + 1 + k])):
                if mutant == "a":
                    fw_len, fw_hit = k, k
                    break
                fw_rej = k
                if mutant == "b":
                    break
        if mutant == "f_add" or (fw_len == bw_len and s[fw_u:fw_u + fw_len] == s[bw_u:bw_u + bw_len]):
            max_rl = max_bw + max_fw
        elif mutant == "f_norecount":
            max_rl = max_fw
        else:
            max_rl = max_fw + _count(s, fw_u, fw_len, 0, offset + 1, False, mutant == "d_before")
    return Scan(min(max_rl, MAX_REPEAT_LENGTH), max_rl, bw_hit, fw_hit, bw_rej if bw_hit else 0, fw_rej if fw_hit else 0)


@functools.lru_cache(maxsize=None)
def repeat_lengths(s, mutant=None):
    """Scan.length at every position of s, as a tuple (the last position included: only mutant g_last looks at it)."""
    return tuple(scan(s, i, mutant).length for i in range(len(s)))


@functools.lru_cache(maxsize=None)
def scans(s):
    return tuple(scan(s, i) for i in range(len(s)))


@functools.lru_cache(maxsize=None)
def cache_of(pcr):
    return tuple(int(x) for x in oracle.pcr_error_model_cache(MODELS[pcr])) if pcr else None


def modify(bases, mapq, q, ins, dele, pcr, bq_threshold, disable_cap, mutant=None):
    """modify_read_qualities restated: (base, insertion, deletion qualities) as lists.  ins / dele None: flat 45."""
    n, s = len(bases), bytes(bases)
    cache = cache_of(pcr)
    rl = repeat_lengths(s, mutant if mutant in SCAN_MUTANTS else None) if cache else None
    oq, oi, od = [], [], []
    for i in range(n):
        b, iq, dq = int(q[i]), DEFAULT_INDEL_Q if ins is None else int(ins[i]), DEFAULT_INDEL_Q if dele is None else int(dele[i])
        if mutant == "h" and i >= 64:
            oq.append(b), oi.append(iq), od.append(dq)
            continue
        if cache and (i < n - 1 or mutant == "g_last"):
            c = cache[rl[i]]
            iq, dq = (c, c) if mutant == "i" else (min(iq, c), min(dq, c))
        if not disable_cap:
            b = min(b, int(mapq))
        if b < bq_threshold:
            b = MIN_USABLE_Q
        oq.append(b), oi.append(max(iq, MIN_USABLE_Q)), od.append(max(dq, MIN_USABLE_Q))
    return oq, oi, od


# engine.rs:23-39, (mean, variance) for base qualities 1 ... 40
DYN_TABLE = ((5.996842844, 0.196616587), (5.870018422, 1.388545569), (5.401558531, 5.641990128), (4.818940919, 10.33176216),
             (4.218758304, 14.25799688), (3.646319832, 17.02880749), (3.122346753, 18.64537883), (2.654731979, 19.27521677),
             (2.244479156, 19.13584613), (1.88893867, 18.43922003), (1.583645342, 17.36842261), (1.3233807, 16.07088712),
             (1.102785365, 14.65952563), (0.916703025, 13.21718577), (0.760361881, 11.80207947), (0.629457387, 10.45304833),
             (0.520175654, 9.194183767), (0.42918208, 8.038657241), (0.353590663, 6.991779595), (0.290923699, 6.053379213),
             (0.23906788, 5.219610436), (0.196230431, 4.484302033), (0.160897421, 3.839943445), (0.131795374, 3.27839108),
             (0.1078567, 2.791361596), (0.088189063, 2.370765375), (0.072048567, 2.008921719), (0.058816518, 1.698687797),
             (0.047979438, 1.433525748), (0.039111985, 1.207526336), (0.031862437, 1.015402928), (0.025940415, 0.852465956),
             (0.021106532, 0.714585285), (0.017163711, 0.598145851), (0.013949904, 0.500000349), (0.011332027, 0.41742159),
             (0.009200898, 0.348056286), (0.007467036, 0.289881373), (0.006057179, 0.241163527), (0.004911394, 0.200422214))


def threshold(q, dynamic, scale, err, mutant=None, modified_q=None):
    """log10_min_true_likelihood / calculate_log10_dynamic_read_qual_threshold / dynamic_log10_min_likelihood_model restated.
    q: the ORIGINAL base qualities (mutant l takes modified_q in their place)."""
    n = len(q)
    x = n * err
    e = math.floor(x) if mutant == "j_floor" else math.floor(x + 0.5) if mutant == "j_round" else math.ceil(x)
    if not dynamic:
        return min(2.0, float(e)) * -4.0
    sum_mean = sum_var = 0.0
    for b in (modified_q if mutant == "l" else q):
        b = int(b)
        idx = 0 if b <= 1 else min(40, b) - 1
        idx = max(0, idx - 1) if mutant == "k_minus" else min(39, idx + 1) if mutant == "k_plus" else idx
        sum_mean += DYN_TABLE[idx][0]
        sum_var += DYN_TABLE[idx][1]
    dyn = (sum_mean + scale * math.sqrt(sum_var)) * -0.1
    cap = float(e) * -4.0
    return max(dyn, cap) if mutant == "m" else (dyn if dyn < cap else cap)


# ---- the host's rules, restated (test_prestep_table.py holds them to phmm_api.cpp, phmm_region.cpp, phmm_engine_kernels.hip) ----
SMALL_CALL_READS = 2048
LDS_BYTES_PER_ROW, WAVES_PER_BLOCK = 17, 4
LDS_DEFAULT_LIMIT, LDS_BYTES_PER_CU = 64 * 1024, 160 * 1024
ONE_SHOT_BYTES = 512 << 10


def waves_per_read(n_reads, longest):
    return max(1, (longest + 63) // 64) if n_reads <= SMALL_CALL_READS else 1


def lds_rows(longest):
    return (longest + 1 + 7) // 8 * 8


def lds_bytes(longest):
    return lds_rows(longest) * LDS_BYTES_PER_ROW * WAVES_PER_BLOCK


# The long reads follow from those rules: the first length whose launch asks for more than the default 64 KiB (so that it goes
# through hipFuncSetAttribute), the longest the host accepts, and one base more.  lds_rows rounds n + 1 up to eight, so the
# first length past 64 KiB is 960 (968 rows, 65 824 bytes; 959 -> 960 rows, 65 280 bytes); 964, the length that
# (n + 1) * 68 > 65536 alone would give after rounding to the next multiple of four, sits in the same block of rows and is kept.
FIRST_OVER_64K = next(n for n in range(1, 4096) if lds_bytes(n) > LDS_DEFAULT_LIMIT)
LONGEST_ACCEPTED = max(n for n in range(1, 4096) if lds_bytes(n) <= LDS_BYTES_PER_CU)
LONG_LENGTHS = (FIRST_OVER_64K - 1, FIRST_OVER_64K, 964, LONGEST_ACCEPTED)
REFUSED_LENGTH = LONGEST_ACCEPTED + 1


# ---- the reads -------------------------------------------------------------------------------------------------------------------
# SEEDS: per region name, the first seed, counted from 0, with which the conditions of tests/test_prestep_table.py hold by the
# oracle alone (a seed that fails is replaced here; no read is ever left out).
SEEDS = {}
LEAD = 192      # bases in front of the first block of a unit region: room to put a block across read position 191|192


def _rng(name):
    return np.random.default_rng(zlib.crc32(repr(("prestep", name, SEEDS.get(name, 0))).encode()))


def _other(b, *avoid):
    return next(x for x in ALPHA if x != b and x not in avoid)


def _unit(rng, L):
    """A unit of L bases that is no repeat of a shorter one.  From 8 bases on its last two bases recur L - 3 positions earlier
    while the third-last does not (and the same read forwards from its second base): a candidate the device's screen passes and
    its exact test rejects, in front of the true length."""
    while True:
        u = bytearray(rnd(rng, L))
        if L == 1:
            return bytes(u)
        if L >= 8:
            u[L - 1], u[L - 2] = u[2], u[1]
            if u[L - 3] == u[0] or u[3] == u[0]:
                continue
        u = bytes(u)
        if all(u != u[:k] * (L // k) for k in range(1, L) if L % k == 0) and len(set(u)) > 1:
            rep = u * 3
            # (no shorter unit is found anywhere inside three copies: every position of the block sees the unit itself)
            if all(scan(rep, i).bw_len in (0, L) and scan(rep, i).fw_len in (0, L) for i in range(len(rep))):
                return u


def _spacer(rng, n, before, after):
    """n random bases that continue neither neighbour."""
    while True:
        sp = bytearray(rnd(rng, n))
        if before and sp[0] == before[-1]:
            sp[0] = _other(before[-1], after[0] if after and n == 1 else 0)
        if after and sp[-1] == after[0]:
            sp[-1] = _other(after[0], before[-1] if before and n == 1 else 0)
        return bytes(sp)


Region = namedtuple("Region", "name haps cigars starts reads notes")   # reads: [bytes]; notes: per read, what it is there for


def _alleles(parts, which, unit):
    """The haplotypes of an STR: `parts` joined is the reference; the alternative ones carry one copy of `unit` (None: one base) more /
    fewer at the start of parts[which[k]] (a block of copies), with the exact CIGARs."""
    ref = b"".join(parts)
    given = unit
    haps, cigs = [ref], ["%dM" % len(ref)]
    for k, w in enumerate(which):
        p = len(b"".join(parts[:w]))
        unit = parts[w][:1] if given is None else given
        if k % 2 == 0:
            haps.append(ref[:p] + unit + ref[p:])
            cigs.append("%dM%dI%dM" % (p, len(unit), len(ref) - p) if p else "%dI%dM" % (len(unit), len(ref)))
        else:
            haps.append(ref[:p] + ref[p + len(unit):])
            cigs.append("%dM%dD%dM" % (p, len(unit), len(ref) - p - len(unit)))
    return haps, cigs


def _unit_region(L):
    """Unit length L with 3, 4 and 6 copies: [lead | 3 copies | spacer | 4 copies | spacer | 6 copies | tail]."""
    name = "unit-%d" % L
    rng = _rng(name)
    u = _unit(rng, L)
    lead = _spacer(rng, LEAD, b"", u)
    s1, s2, tail = _spacer(rng, 9, u, u), _spacer(rng, 9, u, u), _spacer(rng, 12, u, b"")
    parts = [lead, u * 3, s1, u * 4, s2, u * 6, tail]
    haps, cigs = _alleles(parts, (3, 1), u)
    ref = haps[0]
    b1 = LEAD
    e1 = b1 + 3 * L
    b2 = e1 + 9
    e2 = b2 + 4 * L
    b3 = e2 + 9
    e3 = b3 + 6 * L
    cut = lambda h, a, b: h[max(0, a):min(len(h), b, max(0, a) + SRV_MAX_ROWS)]  # noqa: E731
    reads = [(cut(ref, b1, e2 + 5), "start"), (cut(ref, b1 + 1, e2 + 5), "start+1"),
             (ref[max(b2 - 4, e3 - SRV_MAX_ROWS):e3], "end"), (ref[max(b2 - 4, e3 - 1 - SRV_MAX_ROWS):e3 - 1], "end-1"),
             (cut(ref, b1 - 7, b3 + 4), "middle")]
    for x in (64, 128, 192):                       # the second copy of the middle block ends at read position x - 1
        a = b2 + 2 * L - x
        reads.append((cut(ref, a, e2 + 12), "across-%d" % x))
    reads.append((cut(haps[1], b2 - 15, e2 + L + 15), "alt-longer"))
    reads.append((cut(haps[2], b1 - 15, e1 - L + 15 + 20), "alt-shorter"))
    return Region(name, haps, cigs, [0, 0, 0], [r for r, _ in reads], [t for _, t in reads])


def _special_region():
    """Different backward and forward units (same length, different lengths), forward units that also tile what lies behind the
    offset (units that end in a doubled base: the backward search finds the homopolymer first), N and a lower-case base inside
    a repeat."""
    name = "special"
    rng = _rng(name)
    blocks = [b"AC" * 4 + b"GT" * 4, b"ACGGT" * 3 + b"TCAAG" * 3, b"AC" * 4 + b"GCTTGCA" * 3, b"GCTTAA" * 4, b"TGCACGTCC" * 3,
              b"GAA" * 5, b"CTGGATCGATTACGAGCCTT" * 3]
    parts, marks = [_spacer(rng, 14, b"", blocks[0])], []
    for k, blk in enumerate(blocks):
        marks.append((len(b"".join(parts)), len(blk)))
        parts.append(blk)
        parts.append(_spacer(rng, 11, blk, blocks[k + 1] if k + 1 < len(blocks) else b""))
    ref = b"".join(parts)
    p3, p5 = marks[3][0], marks[5][0]
    haps = [ref, ref[:p3] + b"GCTTAA" + ref[p3:], ref[:p5] + ref[p5 + 3:]]
    cigs = ["%dM" % len(ref), "%dM6I%dM" % (p3, len(ref) - p3), "%dM3D%dM" % (p5, len(ref) - p5 - 3)]
    reads, notes = [], []
    for k, (p, ln) in enumerate(marks):
        reads += [ref[p - 9:p + ln + 9], ref[p:p + ln], ref[p - 3:p + ln]]
        notes += ["block-%d" % k, "block-%d-bare" % k, "block-%d-at-end" % k]
    reads += [ref[:SRV_MAX_ROWS], ref[len(ref) - SRV_MAX_ROWS:], haps[1][p3 - 20:p3 + 50], haps[2][p5 - 30:p5 + 30]]
    notes += ["whole-left", "whole-right", "alt-longer", "alt-shorter"]
    p0 = marks[0][0]
    odd = bytearray(ref[p0 - 9:p0 + 16 + 9])
    odd[9 + 4], odd[9 + 11] = ord("N"), ord("t")
    reads.append(bytes(odd))
    notes.append("N-and-lower-case")
    return Region(name, haps, cigs, [0, 0, 0], reads, notes)


RUNS = ((b"A", 99), (b"A", 100), (b"A", 101), (b"A", 150), (b"CA", 101))     # (unit, copies): the cap at 100


def _run_region(unit, copies):
    name = "run-%s-%d" % (unit.decode(), copies * len(unit))
    rng = _rng(name)
    run = unit * copies
    left, right = _spacer(rng, 24, b"", run), _spacer(rng, 24, run, b"")
    haps, cigs = _alleles([left, run, right], (1, 1), unit)
    ref = haps[0]
    a, b = 24, 24 + len(run)
    reads = [(ref[a - 10:b + 10], "flanked"), (ref[a:b], "bare"), (ref[a - 10:b], "at-end"), (ref[a:b + 10], "at-start"),
             (haps[1][a - 10:b + len(unit) + 10], "alt-longer"), (haps[2][a - 10:b - len(unit) + 10], "alt-shorter")]
    return Region(name, haps, cigs, [0, 0, 0], [r[:SRV_MAX_ROWS] for r, _ in reads], [t for _, t in reads])


LADDER = tuple(range(7, 34))     # repeat lengths the unit regions do not reach and the conservative cache still resolves


def _ladder_region(part):
    """Homopolymer runs of 7 ... 33 bases, nine to a haplotype, each in a read of its own."""
    name = "ladder-%d" % part
    rng = _rng(name)
    runs = LADDER[9 * part:9 * part + 9]
    parts = [rnd(rng, 10)]
    for j, k in enumerate(runs):
        base = ALPHA[(j + part) % 4:(j + part) % 4 + 1]
        parts[-1] = parts[-1][:-1] + bytes([_other(parts[-1][-1], base[0])])
        parts.append(base * k)
        sp = bytearray(rnd(rng, 10))
        sp[0] = _other(base[0])
        parts.append(bytes(sp))
    haps, cigs = _alleles(parts, (3, 7), None)
    ref = haps[0]
    reads, notes, p = [], [], 0
    for j, x in enumerate(parts):
        if j % 2:
            reads.append(ref[p - 8:p + len(x) + 8])
            notes.append("run-%d" % len(x))
        p += len(x)
    return Region(name, haps, cigs, [0, 0, 0], reads, notes)


SHORT_LENGTHS = (1, 2, 3, 63, 64, 65, 128, 129, 268)


def _plain_haps(rng, n):
    ref = rnd(rng, n)
    alt = bytearray(ref)
    for p in range(17, n, 41):
        alt[p] = _other(alt[p])
    return [ref, bytes(alt)], ["%dM" % n, "%dM" % n]


def _short_region():
    name = "short"
    rng = _rng(name)
    haps, cigs = _plain_haps(rng, 300)
    reads = [haps[k % 2][5 + 3 * k:5 + 3 * k + n] for k, n in enumerate(SHORT_LENGTHS)]
    return Region(name, haps, cigs, [0, 0], reads, ["length-%d" % n for n in SHORT_LENGTHS])


def _mismatch(read, positions):
    read = bytearray(read)
    for p in positions:
        read[p] = _other(read[p])
    return bytes(read)


STATIC_PAIRS = ((50, 51, 1), (100, 101, 1), (100, 101, 2))      # (n, n + 1, mismatches): the steps of ceil(n * rate)


def _static_region():
    """Pairs of reads of n and n + 1 bases with the same mismatches at Q30: ceil(n * 0.02) steps at 50 | 51 (1 -> 2 errors: the
    static threshold -4 -> -8) and at 100 | 101 (2 -> 3 errors; the static threshold is min(2, errors) * -4 and stays at -8
    there, so that step shows in the dynamic model's cap, errors * -4 = -8 -> -12, and under the static threshold with the
    rate 0.01: 1 -> 2 errors).  A read starts anywhere on its 300-base haplotype, log10(1 / 300) = -2.48, and a mismatch at Q30 costs
    log10(0.001 / 3) = -3.48: with one mismatch the likelihood lies between -4 and -8, with two between -8 and -12."""
    name = "static-steps"
    rng = _rng(name)
    haps, cigs = _plain_haps(rng, 300)
    reads, notes = [], []
    for k, (n, m, mm) in enumerate(STATIC_PAIRS):
        s = 20 + 31 * k
        pos = [9, 30, 44][:mm]
        reads += [_mismatch(haps[0][s:s + n], pos), _mismatch(haps[0][s:s + m], pos)]
        notes += ["pair-%d-%d-%dmm" % (n, m, mm), "pair-%d-%d-%dmm" % (m, n, mm)]
    return Region(name, haps, cigs, [0, 0], reads, notes)


# Dynamic threshold probes: (name, low-quality bases, mismatches on low-quality bases).  The mismatch counts were chosen by
# search with the oracle alone (test_prestep_table.py states the conditions): a mismatch on a base below the score threshold
# costs about 0.95, a match 0.125, so a ladder of counts walks the best likelihood across the read's threshold -- and across
# the thresholds of the mutants k, l and m -- in steps finer than the windows between them.
HIGH_Q = (40, 41, 42, 60, 93, 255)
LOW_Q = (0, 1, 2)
DYN_LENGTH = 120
DYN_PROBES = ([("dyn-high-%d" % m, 0, m) for m in (0, 1, 2, 3)]                      # dyn > cap: the cap decides
              + [("dyn-few-%d" % m, 3, m) for m in (0, 3)]
              + [("dyn-half-%d" % m, 60, m) for m in range(24, 36)]                  # dyn < cap: the table decides
              + [("dyn-q2-%d" % m, 100, m) for m in range(41, 56)]
              + [("dyn-low-%d" % m, 30, m) for m in (0, 4, 8, 12, 16, 20, 24)])      # between cap and dyn for mutants l, m


def dyn_quals(name, low):
    """Base qualities of a dynamic probe: `low` bases from LOW_Q (only 2 for the q2 probes) spread over the read, the rest HIGH_Q."""
    q = np.array([HIGH_Q[i % len(HIGH_Q)] for i in range(DYN_LENGTH)], np.uint8)
    where = np.linspace(0, DYN_LENGTH - 1, low).astype(int) if low else np.zeros(0, int)
    for k, p in enumerate(where):
        q[p] = 2 if name.startswith("dyn-q2") else LOW_Q[k % 3]
    return q, where


def _dynamic_region():
    name = "dynamic-steps"
    rng = _rng(name)
    haps, cigs = _plain_haps(rng, 200)
    reads, notes = [], []
    for k, (probe, low, mm) in enumerate(DYN_PROBES):
        _, where = dyn_quals(probe, low)
        s = 3 + k
        where = list(where) if low else [10, 50, 90, 110]     # (no low-quality base: the mismatches sit on high-quality ones)
        reads.append(_mismatch(haps[k % 2][s:s + DYN_LENGTH], where[:mm]))
        notes.append(probe)
    return Region(name, haps, cigs, [0, 0], reads, notes)


@functools.lru_cache(maxsize=None)
def regions():
    return tuple([_unit_region(L) for L in range(1, MAX_STR_UNIT_LENGTH + 1)] + [_special_region()]
                 + [_run_region(u, c) for u, c in RUNS] + [_ladder_region(k) for k in range(3)] + [_short_region(), _static_region(), _dynamic_region()])


# ---- the configurations: one Case each, the same reads ------------------------------------------------------------------------------
Config = namedtuple("Config", "name tags cfg_kw")
CONFIGS = (Config("hostile-static-tags", True, dict(pcr=1)),
           Config("hostile-dynamic-null", False, dict(pcr=1, dynamic=True, disable_cap=True)),
           Config("aggressive-dynamic-tags", True, dict(pcr=2, dynamic=True, symmetric=False)),
           Config("aggressive-static-null-rate01", False, dict(pcr=2, err=0.01, disable_cap=True)),
           Config("conservative-static-null", False, dict(pcr=3)),
           Config("conservative-dynamic-tags", True, dict(pcr=3, dynamic=True, disable_cap=True)),
           Config("none-static-null", False, dict(pcr=0)),
           Config("none-dynamic-tags", True, dict(pcr=0, dynamic=True, symmetric=False)))
CONFIG_NAMES = tuple(c.name for c in CONFIGS)
MAPQS = (60, 60, 10, 60, 0, 60, 60)


def _base_quals(region, k, read):
    """Base qualities and mapq of read k of a region: the same under every configuration."""
    n = len(read)
    if region.name == "dynamic-steps":
        return dyn_quals(*DYN_PROBES[k][:2])[0], 60
    if region.name == "static-steps" or region.name.startswith("long-"):
        return np.full(n, 30, np.uint8), 60
    rng = np.random.default_rng(zlib.crc32(repr((region.name, k)).encode()))
    q = rng.choice([37, 32, 27, 22, 18, 17, 12, 6, 2], n, p=[.45, .15, .1, .1, .04, .04, .05, .05, .02]).astype(np.uint8)
    return q, MAPQS[(k + len(region.name)) % len(MAPQS)]


def _tags(read, k, pcr):
    """Insertion and deletion tags placed against the cache value of the same position: below it, equal to it, above it, below
    MIN_USABLE_Q, and the default 45, in turn (the deletion tags four steps ahead of the insertion tags)."""
    rl = repeat_lengths(read)
    cache = cache_of(pcr)
    ins, dele = np.zeros(len(read), np.uint8), np.zeros(len(read), np.uint8)
    for i in range(len(read)):
        c = cache[rl[i]] if cache else 30
        ladder = (max(0, c - 3), c, c + 4, DEFAULT_INDEL_Q, c - 1, c + 1, DEFAULT_INDEL_Q, c, 3, DEFAULT_INDEL_Q, max(0, c - 2))
        ins[i], dele[i] = ladder[(i + k) % 11], ladder[(i + k + 4) % 11]
    return ins, dele


def _build(name, regs, config):
    staged = []
    for reg in regs:
        reads = []
        for k, s in enumerate(reg.reads):
            n = len(s)
            # (the static pairs keep the default tags: their likelihood has to lie between two thresholds four apart)
            tagged = config.tags and reg.name != "static-steps"
            ins, dele = _tags(s, k, config.cfg_kw["pcr"]) if tagged else (np.full(n, DEFAULT_INDEL_Q, np.uint8),) * 2
            reads.append(Read(s, _base_quals(reg, k, s)[0], ins, dele, np.full(n, 10, np.uint8)))
        staged.append((reads, list(reg.haps), [oracle.parse_cigar(c) for c in reg.cigars], list(reg.starts),
                       [oracle.parse_cigar("%dM" % len(s)) for s in reg.reads]))
    want = RegionBatch.from_regions([(r[0], r[1]) for r in staged])
    c = _assemble(name, staged, config.cfg_kw, np.random.default_rng(zlib.crc32(name.encode())))
    b = c.batch          # (_assemble spreads qualities of its own over the batch: the designed ones go back in)
    b.base_q[:], b.ins_q[:], b.del_q[:] = want.base_q, want.ins_q, want.del_q
    c.mapq[:] = [_base_quals(reg, k, s)[1] for reg in regs for k, s in enumerate(reg.reads)]
    return c


@functools.lru_cache(maxsize=None)
def case(config_name):
    return _build("prestep-" + config_name, regions(), CONFIGS[CONFIG_NAMES.index(config_name)])


def config_of(c):
    return next(k for k in CONFIGS if c.name.split("[")[0].endswith(k.name))


def uses_tags(c):
    return config_of(c).tags


MULTIPLIED_CONFIG = "hostile-static-tags"


@functools.lru_cache(maxsize=None)
def multiplied_case():
    """The reads of one configuration cycled to just over 2 048 in one call: the engine route with waves_per_read = 1.  Returns
    (case, first: for every region the index of the region it is a copy of)."""
    config = CONFIGS[CONFIG_NAMES.index(MULTIPLIED_CONFIG)]
    regs, first, n = [], [], 0
    while n <= SMALL_CALL_READS:
        reg = regions()[len(regs) % len(regions())]
        first.append(len(regs) % len(regions()))
        regs.append(reg)
        n += len(reg.reads)
    return _build("prestep-multiplied-" + config.name, regs, config), first


@functools.lru_cache(maxsize=None)
def long_case(n):
    """One read of n bases that carries three copies of a 20-base unit near its end, and two haplotypes a little longer."""
    name = "long-%d" % n
    rng = _rng(name)
    u = _unit(rng, 20)
    tail = _spacer(rng, 7, u, b"")
    head = _spacer(rng, n + 10 - 60 - 7, b"", u)
    ref = head + u * 3 + tail + rnd(rng, 8)
    p = len(head)
    haps, cigs = [ref, ref[:p] + u + ref[p:]], ["%dM" % len(ref), "%dM20I%dM" % (p, len(ref) - p)]
    read = ref[10:10 + n]
    reg = Region(name, haps, cigs, [0, 0], [read], ["long"])
    return _build("prestep-" + name, [reg], Config("long-hostile-dynamic-null", False, dict(pcr=1, dynamic=True)))


# ---- the oracle's answer, once per process and case -------------------------------------------------------------------------------
Expected = namedtuple("Expected", "likelihoods keep best")
_expected = {}


def expected(c):
    if c.name not in _expected:
        out, keep, best = _oracle_pipeline(c.cfg, c.batch, c.mapq, c.ref_hap, c.pri)
        for a in (out, keep, best):
            a.setflags(write=False)
        _expected[c.name] = Expected(out, keep, best)
    return _expected[c.name]


def expected_multiplied():
    """The oracle's answer for the multiplied case, from the plain case's: regions are independent, a copy gives its original's rows."""
    c, first = multiplied_case()
    plain, e, b, pb = case(MULTIPLIED_CONFIG), expected(case(MULTIPLIED_CONFIG)), c.batch, case(MULTIPLIED_CONFIG).batch
    out, keep = np.zeros(b.n_out), np.zeros(b.n_reads, bool)
    for g, f in enumerate(first):
        out[int(b.out_off[g]):int(b.out_off[g + 1])] = e.likelihoods[int(pb.out_off[f]):int(pb.out_off[f + 1])]
        keep[int(b.region_read_off[g]):int(b.region_read_off[g + 1])] = e.keep[int(pb.region_read_off[f]):int(pb.region_read_off[f + 1])]
    assert plain.batch.n_regions == len(regions())
    return out, keep


def read_slices(c):
    b = c.batch
    return [(int(b.read_off[r]), int(b.read_off[r + 1])) for r in range(b.n_reads)]


def region_of_reads(b):
    return np.repeat(np.arange(b.n_regions), np.diff(b.region_read_off.astype(np.int64)))


def best_and_threshold(c):
    """Per read: the oracle's best normalised likelihood over the alleles, and the oracle's threshold."""
    b, e = c.batch, expected(c)
    best, thr = np.zeros(b.n_reads), np.zeros(b.n_reads)
    for g in range(b.n_regions):
        r0, r1, nh = int(b.region_read_off[g]), int(b.region_read_off[g + 1]), int(b.region_hap_off[g + 1] - b.region_hap_off[g])
        best[r0:r1] = e.likelihoods[int(b.out_off[g]):int(b.out_off[g + 1])].reshape(r1 - r0, nh).max(axis=1)
    for r, (s, t) in enumerate(read_slices(c)):
        thr[r] = oracle.read_disqualification_threshold(b.base_q[s:t], bool(c.cfg.dynamic_read_disqualification), c.cfg.read_disqualification_scale,
                                                        c.cfg.expected_error_rate_per_base)
    return best, thr


def _modify_args(c, r, s, t):
    b, cfg, tags = c.batch, c.cfg, uses_tags(c)
    return (b.read_bases[s:t].tobytes(), int(c.mapq[r]), b.base_q[s:t], b.ins_q[s:t] if tags else None, b.del_q[s:t] if tags else None,
            cfg.pcr_error_model, cfg.base_quality_score_threshold, bool(cfg.disable_cap_read_qualities_to_mapq))


_right = {}


def right_qualities(c):
    """Per read the restated (q, ins, dele), once per process and case."""
    if c.name not in _right:
        _right[c.name] = [modify(*_modify_args(c, r, s, t)) for r, (s, t) in enumerate(read_slices(c))]
    return _right[c.name]


def mutant_qualities(c, mutant):
    """Per read (q, ins, dele) under the mutant, None where they equal the right ones."""
    good, out = right_qualities(c), []
    for r, (s, t) in enumerate(read_slices(c)):
        args = _modify_args(c, r, s, t)
        if mutant in SCAN_MUTANTS and mutant != "g_last" and repeat_lengths(args[0], mutant) == repeat_lengths(args[0]):
            out.append(None)        # (the same repeat lengths: the same qualities)
            continue
        bad = modify(*args, mutant=mutant)
        out.append(None if good[r] == bad else bad)
    return out


def likelihood_change(c, per_read, at_most=24):
    """The largest change of a normalised likelihood of the case when the reads listed in per_read (read -> (q, ins, dele)) go
    through the oracle with those qualities; the `at_most` reads whose qualities differ most are tried."""
    b, cfg, e = c.batch, c.cfg, expected(c)
    reg = region_of_reads(b)
    sl = read_slices(c)
    good = right_qualities(c)
    weight = {r: sum(abs(x - y) for k in range(3) for x, y in zip(per_read[r][k], good[r][k])) for r in per_read}
    chosen = sorted(per_read, key=lambda r: (-weight[r], r))[:at_most]
    largest, n = 0.0, 0
    for g in sorted({int(reg[r]) for r in chosen}):
        rs = [r for r in chosen if reg[r] == g]
        h0, h1, r0 = int(b.region_hap_off[g]), int(b.region_hap_off[g + 1]), int(b.region_read_off[g])
        haps = [b.hap_bases[int(b.hap_off[a]):int(b.hap_off[a + 1])] for a in range(h0, h1)]
        reads = [Read(b.read_bases[sl[r][0]:sl[r][1]], *(np.array(x, np.uint8) for x in per_read[r]), np.full(sl[r][1] - sl[r][0], cfg.constant_gcp, np.uint8))
                 for r in rs]
        rb = RegionBatch.from_regions([(reads, haps)])
        raw = oracle.compute_batch(rb.as_dict(), n_threads=4).reshape(len(rs), h1 - h0)
        norm = oracle.normalize_likelihoods(raw.T.copy(), cfg.log10_global_read_mismapping_rate, bool(cfg.symmetrically_normalize_alleles_to_reference),
                                            c.ref_hap[g]).T
        want = e.likelihoods[int(b.out_off[g]):int(b.out_off[g + 1])].reshape(-1, h1 - h0)
        for k, r in enumerate(rs):
            largest = max(largest, float(np.max(np.abs(norm[k] - want[r - r0]))))
            n += 1
    return largest, n
