"""What tests/test_activity_wave_hip.py crosses, counted on the CPU from the inputs and the restatement alone
(tests/activity_wave_cases.py): second and later trips of activity_read_kernel's two lane-strided loops per operator kind and
for elements that start before the window, the chunk shapes of activity_site_kernel<CH> at G = 4, 8, 9, 16, 17, both routes
of the allele-frequency step, the launch grids at n_pos and max_prof_n + max_filter_size = 255, 256, 257 (mod 256), and both
ends of `qual as u8`.  Every count is above 0, the long-element and long-clip windows reach theirs without the seeded ones,
and each witness position holds restated values that a loop which stopped after its first trip could not have produced.  The
rules restated here (chunk width, af_is_block_event, the workgroup size) are checked against the source text.  No GPU."""
import math
import os
import random
import re
from collections import Counter

import numpy as np
import pytest

import activity_cases as K
import activity_restatement as R
import activity_wave_cases as W
from conftest import ROOT
from lorikeet_amd import _lib, activity  # noqa: F401

CSRC = os.path.join(ROOT, "lorikeet_amd", "csrc")
THREADS = 256  # ACT_THREADS
EDGE = (255, 0, 1)


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constant(text, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)u?\s*;" % re.escape(name), text)
    assert m, name
    return int(m.group(1))


def chunk_shape(G):
    """(CH, full chunks, genotypes in the last partial chunk) of activity_site_kernel<CH>'s walk over G genotypes."""
    CH = 4 if G <= 4 else 8
    return CH, G // CH, G % CH


def test_the_restated_rules_are_the_sources():
    kernels, host, af = _source("phmm_activity_kernels.hip"), _source("phmm_activity.cpp"), _source("phmm_af.cpp")
    assert _constant(_source("phmm_activity_internal.hpp"), "ACT_THREADS") == THREADS
    assert _constant(_source("phmm_af_internal.hpp"), "AF_BLOCK_PASSES") == W.AF_BLOCK_PASSES
    # one wave per read, every loop of the read kernel strides by the wave
    assert "blockIdx.x * (ACT_THREADS / 64) + (threadIdx.x >> 6)" in kernels
    assert "for (uint32_t j = 0; j < len; j += 64)" in kernels and "for (uint32_t j = j0 + lane; j < j1; j += 64)" in kernels
    assert W.LANES == 64
    # the one template dispatch
    assert re.search(r"if \(p\.G <= 4\) hipLaunchKernelGGL\(activity_site_kernel<4>.*\n\s*else hipLaunchKernelGGL\(activity_site_kernel<8>", kernels)
    assert "for (uint32_t g0 = 0; g0 < G; g0 += CH)" in kernels
    # the two launch grids
    assert "dim3(p.n_pos / ACT_THREADS + 1)" in kernels and "(p.max_prof_n + p.max_filter + ACT_THREADS - 1) / ACT_THREADS" in kernels
    # the route
    assert "uint32_t af_genotypes_per_lane(uint32_t G) { return G <= 64 ? 1 :" in af
    body = re.search(r"bool af_is_block_event\(uint32_t G, uint32_t n_samples\) \{(.*?)\n\}", af, re.S).group(1)
    assert "uint32_t S = 64;" in body and "if (af_genotypes_per_lane(G) == 1)" in body and "while (S < G) S <<= 1;" in body
    assert "return (n_samples + 64 / S - 1) / (64 / S) >= AF_BLOCK_PASSES;" in body
    assert "const bool block = af_is_block_event(G, n_samples);" in host
    assert "a.n_wave_events = block ? 0 : n_pos;" in host and "a.n_block_events = block ? n_pos : 0;" in host


def test_route_pairs_straddle_the_rule():
    lanes = {5: 8, 33: 64, 65: 64}
    for ploidy, wave, block, _, seed in W.ROUTE_PAIRS:
        G = ploidy + 1
        per_pass = 64 // lanes[G]
        assert math.ceil(wave / per_pass) == W.AF_BLOCK_PASSES - 1 and math.ceil(block / per_pass) == W.AF_BLOCK_PASSES
        assert not W.af_is_block_event(G, wave) and W.af_is_block_event(G, block)
        a, b = W.case(W.route_name(ploidy, wave)), W.case(W.route_name(ploidy, block))
        assert a[2] == b[2] and a[1][0][:3] == b[1][0][:3]
        assert a[1][0][3][:7] == b[1][0][3][:7] and len(a[1][0][3]) == wave and len(b[1][0][3]) == block
        assert sum(len(s) for s in a[1][0][3][:7]) >= 14
    for G, S in ((2, 2), (3, 4), (4, 4), (5, 8), (8, 8), (9, 16), (17, 32), (33, 64), (64, 64), (65, 64)):
        per_pass = 64 // S
        for n in range(1, 70):
            assert W.af_is_block_event(G, n) == ((n + per_pass - 1) // per_pass >= 8), (G, n)


# ---- the census ---------------------------------------------------------------------------------------------------------------

def times(t):
    return "2 trips" if t == 2 else ">= 3 trips" if t >= 3 else None


def census(cases):
    c = Counter()
    for name, windows, o in cases:
        r, _ = W.restated(name)
        G, n_samples = o["ploidy"] + 1, len(windows[0][3])
        c["G = %d: (CH, full chunks, remainder) = %s" % (G, chunk_shape(G))] += 1
        c["allele-frequency step: %s route" % ("block" if W.af_is_block_event(G, n_samples) else "wave")] += 1
        n_pos = sum(len(w[1]) for w in windows)
        if n_pos >= 255 and n_pos % THREADS in EDGE:
            c["n_pos = %d (mod 256)" % (n_pos % THREADS)] += 1
            c["n_pos at a grid edge: windows"] += len(windows)
        entries = max(min(o["profile_size"] or len(w[1]), len(w[1])) for w in windows) + o["max_filter_size"]
        if entries >= 255 and entries % THREADS in EDGE:
            c["max_prof_n + max_filter_size = %d (mod 256)" % (entries % THREADS)] += 1
            c["list entries behind such a profile's positions that are not zero"] += sum(
                int(np.count_nonzero(p[min(o["profile_size"] or len(p), len(windows[w][1])):])) for p, w in zip(r["profiles"], r["profile_window"]))
        c["profile boundary inside a window"] += bool(o["profile_size"]) and any(o["profile_size"] < len(w[1]) for w in windows)
        q = r["qual"]
        with np.errstate(invalid="ignore"):
            c["QUAL >= 255 and finite"] += int(np.sum((q >= 255.0) & np.isfinite(q)))
            c["QUAL infinite"] += int(np.sum(np.isinf(q)))
            c["QUAL not above 0"] += int(np.sum(~(q > 0.0)))
        c["mult > 1"] += int(np.sum(r["mult"] > 1))
        for w, (start, ref, contig, samples) in enumerate(windows):
            if r["window_status"][w] != 0:
                continue
            for reads in samples:
                for read in reads:
                    seen = set()
                    for op, n in R.parse_cigar(read[1]):
                        if op == "S" and times(W.trips(n)):
                            c["soft-clip count, S element: %s" % times(W.trips(n))] += 1
                            seen.add("soft-clip count, reads: %s" % times(W.trips(n)))
                    for op, n, j0, j1, _ in W.elements(read, start, min(start + len(ref), contig)):
                        t = times(W.trips(j1 - j0))
                        if t:
                            c["slot writing, %s element: %s" % (op, t)] += 1
                            seen.add("slot writing, reads: %s" % t)
                            if j0 > 0:
                                c["slot writing, j0 > 0: %s" % t] += 1
                            if j1 < n:
                                c["slot writing, cut by bound_end: %s" % t] += 1
                    c.update(seen)
    return c


TRIP_LINES = ["soft-clip count, S element: %s" % t for t in ("2 trips", ">= 3 trips")] + \
             ["soft-clip count, reads: %s" % t for t in ("2 trips", ">= 3 trips")] + \
             ["slot writing, %s: %s" % (k, t) for k in ("M element", "= element", "X element", "D element", "reads", "j0 > 0", "cut by bound_end")
              for t in ("2 trips", ">= 3 trips")]
CHUNKS = {4: (4, 1, 0), 8: (8, 1, 0), 9: (8, 1, 1), 16: (8, 2, 0), 17: (8, 2, 1)}
CALL_LINES = ["G = %d: (CH, full chunks, remainder) = %s" % (G, s) for G, s in sorted(CHUNKS.items())] + \
             ["allele-frequency step: wave route", "allele-frequency step: block route"] + \
             ["n_pos = %d (mod 256)" % k for k in EDGE] + ["max_prof_n + max_filter_size = %d (mod 256)" % k for k in EDGE] + \
             ["list entries behind such a profile's positions that are not zero", "profile boundary inside a window",
              "QUAL >= 255 and finite", "QUAL infinite", "QUAL not above 0", "mult > 1"]


def test_census_of_the_wave_cases():
    for G, shape in CHUNKS.items():
        assert chunk_shape(G) == shape
    total = census(W.all_cases())
    print("\nthe wave cases: %d calls" % len(W.all_cases()))
    for k in sorted(total):
        print("  %-72s %6d" % (k, total[k]))
    for line in TRIP_LINES + CALL_LINES:
        assert total[line] > 0, line
    assert total["n_pos at a grid edge: windows"] >= 3 * 4  # several windows per call: window_of is crossed too
    # the hand-made windows reach every trip count on their own, and so do the seeded ones for what real reads are made of
    hand = census(W.group("long") + W.group("clips"))
    print("of these, the one-read windows alone:")
    for line in TRIP_LINES:
        print("  %-72s %6d" % (line, hand[line]))
        assert hand[line] > 0, line
    drawn = census(W.group("seeded"))
    for line in TRIP_LINES:
        if "= element" not in line and "X element" not in line:
            assert drawn[line] > 0, ("seeded", line)
    for G in CHUNKS:
        assert any(o["ploidy"] + 1 == G for _, _, o in W.group("seeded")), G
    # every element length the one-read windows are there for
    ops = Counter()
    for name, windows, _ in W.group("long") + W.group("clips"):
        assert sum(len(s) for w in windows for s in w[3]) == 1, name
        ops.update(R.parse_cigar(windows[0][3][0][0][1]))
    for op in "M=X":
        for n in (63, 64, 65, 128, 129, 200):
            assert ops[(op, n)] > 0, (op, n)
    for n in (64, 65, 130):
        assert ops[("D", n)] > 0, n
    for n in W.CLIP_LENGTHS:
        assert ops[("S", n)] >= 4, n  # leading and trailing, two quality layouts


def test_the_inputs_keep_qual_and_the_flags_clear_of_their_thresholds():
    """The two conditions of test_activity_oracle.py's census, which let QUAL carry a tolerance at all."""
    for name, windows, o in W.all_cases():
        r, _ = W.restated(name)
        assert not np.any(r["window_status"]), name
        q = r["qual"]
        with np.errstate(invalid="ignore"):
            near = np.abs(q - np.round(q)) <= 1e-6
        assert not np.any(near & (np.round(q) >= 1) & (np.round(q) <= 255)), (name, q[near])
        assert np.all(r["margin"] > 1e-9), (name, r["margin"].min())
    r = W.restated("forty Q40 mismatches on one position")[0]
    for at in (W.QUAL_AT, W.QUAL_DEEP_AT):
        assert 255.0 <= r["qual"][at] < np.inf and r["af_flags"][at] & 1 and r["is_active_prob"][at] == np.float32(R.qual_to_prob(255))
    assert np.isinf(r["qual"][W.QUAL_AT + 1]) and not r["af_flags"][W.QUAL_AT + 1] & 1  # forty matching bases: monomorphic, p(variant) = 0
    r = W.restated("eighty matching reads and a threshold below 0")[0]
    assert r["qual"][W.QUAL_AT] == 0.0 and r["af_flags"][W.QUAL_AT] & 1 and r["is_active_prob"][W.QUAL_AT] == 0.0


# ---- the witnesses -----------------------------------------------------------------------------------------------------------

def entry(window, at, ploidy=2):
    lk, clips = W.pileup(window, ploidy)
    r = lk[0][at]
    return (r.read_counts, r.ref_depth, r.non_ref_depth, tuple(r.genotype_likelihoods))


def test_long_element_witnesses():
    """The position is covered by the one read alone, and by another entry once a single base (or the one deletion) of the
    read is changed: the arrays there follow from that base, at an element offset a first trip does not reach."""
    second = 0
    for name, windows, o in W.group("long"):
        r, _ = W.restated(name)
        start, ref, contig, samples = windows[0]
        read = samples[0][0]
        found = [w for w in W.WITNESS[name] if w["kind"] == "long"]
        assert found, name
        for w in found:
            at = w["at"]
            assert r["read_counts"][at, 0] == 1, (name, at)
            spans = [(j0, j1, pos) for _, _, j0, j1, pos in W.elements(read, start, start + len(ref)) if pos + j0 <= start + at < pos + j1]
            assert len(spans) == 1, (name, at)
            j0, j1, pos = spans[0]
            assert (start + at - pos >= j0 + W.LANES) == w["second_trip"], (name, at)
            second += w["second_trip"]
            before, after = entry(windows[0], at), entry(w["changed"], at)
            assert before[0] == after[0] == 1 and before[1:] != after[1:], (name, at, before, after)
            assert (r["read_counts"][at, 0], r["ref_depth"][at, 0], r["non_ref_depth"][at, 0], tuple(r["gl"][at, 0])) == before, (name, at)
        longest = max(j1 - j0 for _, _, j0, j1, _ in W.elements(read, start, start + len(ref)))
        assert (longest > W.LANES) == any(w["second_trip"] for w in found), name  # every case that has a second trip names it
    assert second >= 20


def test_late_clip_witnesses():
    later = 0
    for name, windows, o in W.group("clips"):
        r, _ = W.restated(name)
        pos, cigar, bases, quals = windows[0][3][0][0]
        at_q, high = 0, None
        for op, n in R.parse_cigar(cigar):
            if op == "S":
                high = [q > R.HQ_BASE_QUALITY_SOFTCLIP_THRESHOLD for q in quals[at_q:at_q + n]]
            at_q += n
        (w,) = W.WITNESS[name]
        assert w["count"] == sum(high) and w["first_trip_alone"] == sum(high[:W.LANES]), name
        assert r["soft_clip_count"][w["at"]] == 1 and r["soft_clip_mean"][w["at"]] == float(w["count"]), (name, w["at"])
        assert r["soft_clip_count"].sum() == 1, name
        if len(high) > W.LANES:
            assert w["count"] != w["first_trip_alone"], name
            later += 1
            if "from offset 64" in name:
                assert w["first_trip_alone"] == 0 and w["count"] == len(high) - W.LANES
    assert later == 8  # 65 and 130 bases, leading and trailing, two layouts
    # 5S128M3I64M70S: both clips count, the second over two trips
    r = W.restated("5S128M3I64M70S")[0]
    assert sorted(r["soft_clip_mean"][r["soft_clip_count"] > 0].tolist()) == [75.0, 75.0]


def test_the_threshold_hangs_on_the_late_clip_bases():
    (high, _, _), (low, _, _) = W.threshold()
    a, b = W.restated(high)[0], W.restated(low)[0]
    at = W.THRESHOLD_AT
    assert a["soft_clip_mean"][at] == 6.0 and a["mult"][at] == 13 and a["is_active_prob"][at] > 0
    assert b["soft_clip_mean"][at] == 0.0 and b["mult"][at] == 1 and b["is_active_prob"][at] == a["is_active_prob"][at]
    assert a["soft_clip_count"][at] == b["soft_clip_count"][at] == 5
    assert len(a["profiles"][0]) == len(b["profiles"][0]) and not np.array_equal(a["profiles"][0], b["profiles"][0])


# ---- the host-made table and the restatement itself ------------------------------------------------------------------------------

@pytest.mark.parametrize("ploidy", [7, 8, 15, 16, 32])
def test_term_table_equals_the_restatement(ploidy):
    t = np.zeros((2, 256, ploidy + 1))
    assert _lib.load().phmm_activity_term_table(ploidy, t.ctypes.data_as(_lib.f64p)) == _lib.PHMM_OK
    want = R.term_table(ploidy)
    assert t.tobytes() == want.tobytes(), np.argwhere(t != want)[:5]


REF = K.reference(random.Random(31), 200)
LOG3 = math.log10(3.0)


@pytest.mark.parametrize("ploidy", [1, 2, 3, 8])
def test_one_long_read_in_closed_form(ploidy):
    """test_activity_oracle.py's hand-worked pileup with a 130M read and a 70S60M read: the restatement, too, is held to
    elements longer than 64 bases."""
    right, wrong = math.log10(1.0 - 10.0 ** -3.0), 30 * -0.1 + -LOG3
    lp = math.log10(float(ploidy))
    as_ref, as_alt = (0.0 + (right + lp)) - 1.0 * lp, (0.0 + (wrong + lp)) - 1.0 * lp

    def pile(read):
        lk, clips = R.update_activity_profile([[R.Record(*read)]], REF, 100, len(REF), 10000, ploidy, 10)
        return lk[0], clips

    lk, clips = pile((105, "130M", REF[5:135], [30] * 130))
    for p, r in enumerate(lk):
        inside = 5 <= p < 135
        assert (r.read_counts, r.ref_depth, r.non_ref_depth) == ((1, 1, 0) if inside else (0, 0, 0)), p
        assert clips[p].obs_count == 0
        if inside:
            assert r.genotype_likelihoods[0] == as_ref and r.genotype_likelihoods[ploidy] == as_alt, p
        else:
            assert r.genotype_likelihoods == [0.0] * (ploidy + 1), p
    lk, clips = pile((120, "70S60M", b"T" * 70 + REF[20:80], [30] * 130))
    for p, r in enumerate(lk):
        inside = 20 <= p < 80
        alt = p == 20  # beside the soft clip
        assert (r.read_counts, r.ref_depth, r.non_ref_depth) == ((1, 0, 1) if alt else (1, 1, 0) if inside else (0, 0, 0)), p
        if inside:
            assert r.genotype_likelihoods[0] == (as_alt if alt else as_ref) and r.genotype_likelihoods[ploidy] == (as_ref if alt else as_alt), p
        assert (clips[p].obs_count, clips[p].mean()) == ((1, 70.0) if alt else (0, 0.0)), p
