"""Every compiled instance of the Smith-Waterman kernel (phmm_sw_kernels.hip: PHMM_SW_LIST, PHMM_SW_LIST_T, each also as the
tags-only first pass, and the wide one) against the oracle, at the lengths where its own code differs from its neighbours':
the shortest and the longest alternate that select its K, a partly and a completely filled last lane, lanes without columns,
idle groups in the last wave, gaps longer than a lane's K columns and -- for the largest K of each lane count -- two and three
strips with gaps across the strip edge.  After every call the statistic "sw_instance" must name the instance the case is
for: a case that lands elsewhere fails.  Integer work: CIGAR and offset are EQUAL to the oracle's, for every alignment.

The tables and the batch generator are plain Python (no GPU needed to import them): tests/test_sw_instance_table.py holds
them against the kernel source and checks the generated lengths on the CPU."""
import zlib

import numpy as np
import pytest

from lorikeet_amd.smith_waterman import NEW_SW_PARAMETERS, SW_LITE, SW_WIDE, Parameters, SmithWatermanAligner, last_instance
from oracle import oracle

# <lanes per alignment, columns per lane>, as instantiated (PHMM_SW_LIST) ...
SW_LIST = ((16, 2), (16, 4), (16, 6), (16, 8), (16, 10), (16, 12), (16, 14), (16, 16), (16, 20), (16, 24), (16, 28), (16, 32),
           (8, 4), (8, 8), (8, 12), (8, 16), (8, 19), (8, 22), (8, 26), (8, 32),
           (32, 3), (32, 4), (32, 5), (32, 6), (32, 8), (32, 12), (32, 16),
           (64, 2), (64, 3), (64, 4), (64, 6), (64, 8))
# ... <64 lanes, rows per lane> of the sweep along the alternate (PHMM_SW_LIST_T) ...
SW_LIST_T = ((64, 2), (64, 3), (64, 4), (64, 5), (64, 6), (64, 8))
# ... and the planner's own lists of K per lane count (kSwK16, kSwK8, kSwK32, kSwK64, kSwK64T)
SW_K = {16: (2, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32), 8: (4, 8, 12, 16, 19, 22, 26, 32), 32: (3, 4, 5, 6, 8, 12, 16),
        64: (2, 3, 4, 6, 8)}
SW_K_T = (2, 3, 4, 5, 6, 8)
# Every (L, K, transposed) x (full instance, tags-only first pass).  Nothing is left out: the planner honours a forced lane
# count for every length (phmm_sw.cpp, sw_plan: `force_L`), eight lanes included, as long as a block's LDS holds one
# alignment, which is thousands of bases away from anything here.
CASES = [(L, K, False, lite) for L, K in SW_LIST for lite in (False, True)] + [(L, K, True, lite) for L, K in SW_LIST_T for lite in (False, True)]

STRATEGIES = ("SoftClip", "InDel", "LeadingInDel", "Ignore")
LITE_STRATEGIES = ("SoftClip", "Ignore")     # the tags-only first pass exists for these two (phmm_sw.cpp, sw_run: `lite`)
# the production weights; ties everywhere; gap extension 0
WEIGHTS = (NEW_SW_PARAMETERS, Parameters(1, -1, -1, -1), Parameters(1, -3, -2, 0))

ALPHA = b"ACGT"


def k_list(L, transposed):
    return SW_K_T if transposed else SW_K[L]


def k_prev(L, K, transposed):
    """The next smaller listed K (0 for the first): lengths of L * k_prev + 1 ... L * K select K."""
    ks = k_list(L, transposed)
    i = ks.index(K)
    return ks[i - 1] if i else 0


def _rnd(rng, n, letters=4):
    return bytes(ALPHA[int(x)] for x in rng.integers(0, letters, n))


def _substitute(rng, seq, rate=0.04):
    """Substitutions only, at least one that changes a base (so that the sequence is no exact substring of its source)."""
    out = bytearray(seq)
    hits = [i for i in range(len(out)) if rng.random() < rate] or [len(out) // 2]
    for i in hits:
        out[i] = ALPHA[(ALPHA.index(bytes([out[i]])) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(out)


def _fit(rng, seq, length, letters=4):
    """Exactly `length` bases: cut at the end, or unrelated bases in front and behind (overhangs on both ends)."""
    if len(seq) >= length:
        return seq[:length]
    lack = length - len(seq)
    return _rnd(rng, lack // 2, letters) + seq + _rnd(rng, lack - lack // 2, letters)


def _pair(rng, n, m, kind, gap, at=None):
    """(sweep, laned): `sweep` of n bases is the sequence the kernel walks along, `laned` of exactly m bases the one whose
    positions are shared out over the lanes.  `gap` bases are missing from / added to `laned` (kinds "del" / "ins"), at
    position `at` of it where given."""
    letters = 2 if kind == "two" else 4
    sweep = b"A" * n if kind == "homo" else _rnd(rng, n, letters)
    if kind == "unrelated":
        return sweep, _rnd(rng, m)
    if kind == "homo":       # one letter with an island of another: every cell a tie
        laned = bytearray(b"A" * m)
        for i in range(m // 3, min(m, m // 3 + 1 + m // 5)):
            laned[i] = ord("C")
        return sweep, bytes(laned)
    if kind == "exact":      # an exact substring (SoftClip / Ignore take the shortcut, the other two run the matrix)
        s = int(rng.integers(0, max(1, n - m + 1)))
        return sweep, _fit(rng, sweep[s:s + m], m)
    s = int(rng.integers(0, max(1, min(n // 4, 12) + 1)))
    core = sweep[s:]
    if kind == "ins" and m > gap + 8:
        cut = min(len(core), m - gap)
        p = min(at if at is not None else cut // 2, cut - 2)
        p = max(p, 2)
        laned = _substitute(rng, core[:p]) + _rnd(rng, gap) + _substitute(rng, core[p:cut])
    elif kind == "del" and len(core) > gap + 8:
        p = max(2, min(at if at is not None else (len(core) - gap) // 2, len(core) - gap - 2))
        laned = _substitute(rng, core[:p]) + _substitute(rng, core[p + gap:])
    else:                    # "read", "two": substitutions only
        laned = _substitute(rng, core)
    return sweep, _fit(rng, laned, m, letters)


def _orient(pairs, transposed):
    """(reference, alternate): the alternate's columns are shared out over the lanes, the reference's rows in the sweep along the alternate."""
    return [(laned, sweep) if transposed else (sweep, laned) for sweep, laned in pairs]


def make_batches(L, K, transposed):
    """The calls of one instance -> {"main": pairs, "boundary": pairs, "strips": pairs or None}, pairs = (reference, alternate).

    Lengths are those of the sequence that is shared out over the lanes -- the alternate; the reference for the sweep along
    the alternate -- against the strip of L * K:
      main      the longest is L * K; with it L * Kprev + 1, L * K - 1, lengths around K and L, and 1; the other sequence has
                1, 2, L - 1, L, L + 1 (the skew) and a few hundred bases; every kind of content at the boundary lengths
      boundary  ONE alignment whose length is L * Kprev + 1: the shortest that selects this K
      strips    (largest K of a lane count, not transposed) L * K + 1, 2 L K and 2 L K + 1 next to one-strip alignments, with
                insertions and deletions at the strip edges"""
    rng = np.random.default_rng(zlib.crc32(b"%d,%d,%d" % (L, K, transposed)))
    kp = k_prev(L, K, transposed)
    full, gap = L * K, K + 3                            # a gap longer than one lane's cells
    small_other = (1, 2, L - 1, L, L + 1)
    boundary = [x for x in (L * kp + 1, full - 1, full) if x >= 1]
    ragged = sorted({min(max(x, 1), full) for x in (1, 2, K - 1, K, K + 1, 2 * K - 1, 2 * K + 1, 3 * K, L - 1, L, L + 1, full // 2,
                                                    (L // 2) * K + 1, full - K - 1, full - K, full - K + 1)})
    kinds = ("read", "ins", "del", "unrelated", "two", "homo", "exact")
    main = []
    for m in boundary:
        for kind in kinds:
            n = {"read": m + 37, "ins": max(40, m - 25), "del": m + gap + 29, "unrelated": 333, "two": m + 11, "homo": max(3, m - 7),
                 "exact": m + 60}[kind]
            main.append(_pair(rng, n, m, kind, gap))
        for n in small_other:
            main.append(_pair(rng, n, m, "unrelated" if n < 3 else "read", gap))
        main.append(_pair(rng, m + 2 * gap + 50, m, "ins", gap, at=max(2, m - gap - 4)))   # an insertion that ends in the last lane
    for q, m in enumerate(ragged):
        main.append(_pair(rng, (97, 150, 260, 400)[q % 4], m, kinds[q % len(kinds)], gap))
        main.append(_pair(rng, small_other[q % 5], m, "read", gap))
    per_wave = 64 // L
    if len(main) % per_wave == 0:                       # idle groups in the last wave
        main.append(_pair(rng, 150, max(1, full // 3), "read", gap))
    strips = None
    if K == k_list(L, transposed)[-1] and not transposed:
        strips = []
        for m in (full + 1, 2 * full, 2 * full + 1):
            strips.append(_pair(rng, m + 40, m, "read", gap))
            strips.append(_pair(rng, m + 40, m, "ins", gap, at=full - gap // 2))            # an insertion across the first strip edge
            strips.append(_pair(rng, m + 40, m, "ins", 3, at=full - 1))                     # ... and one that ends right behind it
            strips.append(_pair(rng, m + gap + 60, m, "del", gap, at=full))                 # a deletion in the edge column
            strips.append(_pair(rng, 260, m, "unrelated", gap))
            strips.append(_pair(rng, max(4, m - 30), m, "two", gap))
            strips.append(_pair(rng, L + 1, m, "read", gap))
            if m > 2 * full:
                strips.append(_pair(rng, m + 60, m, "ins", gap, at=2 * full - gap // 2))    # across the second edge
        for m in (1, K + 1, full // 2 + 1, full - 1, full):                                 # one strip, in the same waves
            strips.append(_pair(rng, 150, m, "read", gap))
            strips.append(_pair(rng, 120, m, "ins", gap))
        if len(strips) % per_wave == 0:
            strips.append(_pair(rng, 99, full + 2, "read", gap))
    one = [_pair(rng, 200, L * kp + 1, "ins" if L * kp + 1 > gap + 8 else "read", gap)]
    return {"main": _orient(main, transposed), "boundary": _orient(one, transposed), "strips": _orient(strips, transposed) if strips else None}


def laned_length(pair, transposed):
    """The length the planner picks K by: the alternate's, or the reference's for the sweep along the alternate."""
    return len(pair[0]) if transposed else len(pair[1])


def expected_instance(L, K, transposed, variant, pairs):
    longest = max(laned_length(p, transposed) for p in pairs)
    return {"L": L, "K": K, "transposed": transposed, "variant": variant, "strips": 1 if transposed else -(-longest // (L * K))}


def case_id(case):
    L, K, transposed, lite = case
    return "%s%d-K%d-%s" % ("T" if transposed else "L", L, K, "tags" if lite else "full")


# ---- the GPU side -----------------------------------------------------------------------------------------------------

_want = {}   # (instance) -> {(call, weights, strategy): [(cigar, offset)]}: the full instance and its tags-only twin share the oracle's work


def _oracle(key, call, pairs, prm, strategy):
    if key not in _want:
        _want.clear()
        _want[key] = {}
    k2 = (call, prm.match_value, prm.mismatch_penalty, prm.gap_open_penalty, prm.gap_extend_penalty, strategy)
    if k2 not in _want[key]:
        w = [prm.match_value, prm.mismatch_penalty, prm.gap_open_penalty, prm.gap_extend_penalty]
        _want[key][k2] = [oracle.sw_align(r, a, w, strategy) for r, a in pairs]
    return _want[key][k2]


def _ran(engine, want, ctx):
    got = last_instance(engine)
    assert got is not None and {k: got[k] for k in want} == want, ("another instance ran", ctx, got, want)


def _check(got, want, pairs, ctx):
    assert len(got) == len(want) == len(pairs)
    for k, (g, (cig, off)) in enumerate(zip(got, want)):
        assert g.alignment_offset == off and np.array_equal(g.elements, cig), \
            (ctx, k, len(pairs[k][0]), len(pairs[k][1]), g, oracle.cigar_to_string(cig), off)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_instance_equals_the_oracle(hip_engine, case):
    L, K, transposed, lite = case
    aligner = SmithWatermanAligner(hip_engine)
    batches = make_batches(L, K, transposed)
    variant = SW_LITE if lite else 0
    strategies = LITE_STRATEGIES if lite else STRATEGIES
    key = (L, K, transposed)
    try:
        hip_engine.set_switch("sw_lanes", L)
        hip_engine.set_switch("sw_transpose", 1 if transposed else 0)
        hip_engine.set_switch("sw_lite", 1 if lite else 0)
        for call in ("main", "strips", "boundary"):
            pairs = batches[call]
            if pairs is None:
                continue
            want_inst = expected_instance(L, K, transposed, variant, pairs)
            for prm in WEIGHTS if call != "boundary" else WEIGHTS[:1]:
                for strategy in strategies:
                    ctx = (case_id(case), call, prm.match_value, prm.gap_extend_penalty, strategy)
                    got = aligner.align_batch(pairs, prm, strategy, capacity=256)
                    _ran(hip_engine, want_inst, ctx)
                    if lite and call != "boundary":
                        # both halves of the two passes happen: alignments written from the start cell alone, and alignments
                        # that met a gap and went through the full instance of the same geometry again
                        again = hip_engine.stat("sw_second_pass")
                        assert 0 < again < len(pairs), (ctx, again)
                        second = last_instance(hip_engine, second=True)
                        assert second is not None and (second["L"], second["K"], second["transposed"], second["variant"]) == (L, K, transposed, 0), (ctx, second)
                    elif not lite:
                        assert hip_engine.stat("sw_second_pass") == 0 and last_instance(hip_engine, second=True) is None
                    _check(got, _oracle(key, call, pairs, prm, strategy), pairs, ctx)
    finally:
        hip_engine.set_switch("sw_lite", -1)
        hip_engine.set_switch("sw_transpose", -1)
        hip_engine.set_switch("sw_lanes", 0)


# Weights beyond the scaled kernels' range take the one wide instance, <16, 16> with un-scaled scores: wide while
# |weight| x (ref + alt + 2) >= 1e8, refused from 1e9 (phmm_sw.cpp, sw_plan) -- with 800 000 that is 123 ... 1 247 bases.
WIDE_WEIGHTS = (Parameters(400000, -600000, -800000, -200000), Parameters(3, -800000, -700000, -400000))


def make_wide_batches():
    """The wide instance's calls: the longest alternate is 300 (two strips of 256, the last lane of the second partly filled) /
    513 (three strips, one column in the third); alternates of 255, 256 and 257 columns and short ones beside them."""
    rng = np.random.default_rng(1616)
    out = {}
    for name, longest in (("two_strips", 300), ("three_strips", 513)):
        pairs = []
        for m in (longest, 255, 256, 257, 1, 15, 16, 17, 100) + ((511, 512) if longest > 512 else ()):
            pairs.append(_pair(rng, min(m + 40, 420), m, "read", 19))
            pairs.append(_pair(rng, min(m + 40, 420), m, "ins", 19, at=256 - 9 if m > 280 else None))
            pairs.append(_pair(rng, min(m + 70, 420), m, "del", 19, at=256 if m > 280 else None))
            pairs.append(_pair(rng, (1, 2, 15, 16, 17, 200)[len(pairs) % 6], m, "unrelated", 19))
        pairs.append(_pair(rng, 300, 200, "two", 19))
        if len(pairs) % 4 == 0:
            pairs.append(_pair(rng, 120, 90, "homo", 19))
        out[name] = _orient(pairs, False)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("call", ("two_strips", "three_strips"))
def test_wide_instance_equals_the_oracle(hip_engine, call):
    aligner = SmithWatermanAligner(hip_engine)
    pairs = make_wide_batches()[call]
    want_inst = expected_instance(16, 16, False, SW_WIDE, pairs)
    assert want_inst["strips"] == {"two_strips": 2, "three_strips": 3}[call]
    for prm in WIDE_WEIGHTS:
        for strategy in STRATEGIES:
            ctx = ("wide", call, prm.match_value, strategy)
            got = aligner.align_batch(pairs, prm, strategy, capacity=256)
            _ran(hip_engine, want_inst, ctx)
            w = [prm.match_value, prm.mismatch_penalty, prm.gap_open_penalty, prm.gap_extend_penalty]
            _check(got, [oracle.sw_align(r, a, w, strategy) for r, a in pairs], pairs, ctx)
