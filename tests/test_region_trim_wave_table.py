"""What tests/test_region_trim_wave_hip.py crosses, counted on the CPU from the inputs and the restatement alone
(tests/region_trim_wave_cases.py): passes of compare() behind its first 256 bytes and decisions of its fourth ballot, failing
event maps and trim panics at haplotype 64 and later, calls of more than 1024 regions.  Every count is above 0 on the new sets and
0 on region_trim_cases.sets() with exhaustive_set(); each witness is a set whose restated result a compare() of 192 or 256 bytes,
a search of one trip or a scan of one region a thread could not have given.  The restated loop headers and the three sizes are read
out of the source text: when one is rewritten, the set list needs another look.  No GPU."""
import os
import re
import time

import events_restatement as EV
import region_trim_cases as K
import region_trim_restatement as R
import region_trim_wave_cases as W
from conftest import ROOT
from lorikeet_amd import _lib

CSRC = os.path.join(ROOT, "lorikeet_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constant(text, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)u?\s*;" % re.escape(name), text)
    assert m, name
    return int(m.group(1))


def test_the_restated_loops_are_the_sources():
    kernels, internal = _source("phmm_trim_kernels.hip"), _source("phmm_trim_internal.hpp")
    once = ("for (uint32_t c = 0; c < la; c += 256) {",
            "const uint32_t o = c + q * 64 + lane;",
            "const uint32_t k = c + q * 64 + (uint32_t)__builtin_ctzll(diff);",
            "for (uint32_t base = h0; base < h1 && !status; base += 64) {",
            "if (bad) status = p.hap_status[base + (uint32_t)__builtin_ctzll(bad)];",
            "for (uint32_t base = 0; base < nh && at == TRIM_NONE; base += 64) {",
            "if (bad) at = base + (uint32_t)__builtin_ctzll(bad);",
            "const uint32_t t = threadIdx.x, chunk = (n + TRIM_SCAN_THREADS - 1) / TRIM_SCAN_THREADS;",
            "const uint32_t lo = min(n, t * chunk), hi = min(n, lo + chunk);",
            "const uint32_t n_out = trim_block_scan(p.region_n_out, p.out_region_hap_off, p.n_regions, sums);",
            "__shared__ uint32_t smaller[EV_MAX_HAPS], rep[EV_MAX_HAPS];  // per haplotype: surviving haplotypes below it; its class's representative")
    for line in once:
        assert kernels.count(line) == 1, line
    assert kernels.count("for (uint32_t q = 0; q < 4; ++q) {") == 2          # the loads, then the ballots in byte order
    assert kernels.count("for (uint32_t i = t; i < nh; i += TRIM_RANK_THREADS)") == 3
    assert "__launch_bounds__(64) void trim_span_kernel" in kernels and "__launch_bounds__(64) void trim_rank_kernel" in kernels
    assert W.PASS == 4 * W.LANES == 256
    assert _constant(internal, "TRIM_RANK_THREADS") == 256
    assert _constant(internal, "TRIM_SCAN_THREADS") == 1024
    assert _constant(_source("phmm_events_internal.hpp"), "EV_MAX_HAPS") == _lib.PHMM_EVENTS_MAX_HAPS == 512


def add(total, c):
    for k, v in c.items():
        total[k] += v


def test_census_of_the_wave_sets_and_of_the_first_suite():
    t0 = time.perf_counter()
    total = dict.fromkeys(W.COUNTS, 0)
    by_set = {}
    for name, make in W.SETS.items():
        by_set[name] = W.census(make()["regions"], W.restated_regions(name))
        add(total, by_set[name])
    n_regions = sum(len(make()["regions"]) for make in W.SETS.values())
    print("\nthe wave sets of phmm_trim_regions: %d regions, restated in %.1f s" % (n_regions, time.perf_counter() - t0))
    for k in W.COUNTS:
        print("  %-82s %6d" % (k, total[k]))
        assert total[k] > 0, k
    t0 = time.perf_counter()
    old = dict.fromkeys(W.COUNTS, 0)
    for s in list(K.sets().values()) + [K.exhaustive_set()]:
        add(old, W.census(s["regions"], [R.trim_region(rg, s["dist"], s["padding"]) for rg in s["regions"]], s["dist"]))
    print("the first suite's sets with the exhaustive one: restated in %.1f s" % (time.perf_counter() - t0))
    for k in W.COUNTS:
        assert old[k] == 0, (k, old[k])
    # each set is there for counts of its own
    c = by_set["late_difference"]
    assert c[W.COUNTS[0]] > 0 and c[W.COUNTS[1]] == 2 and c[W.COUNTS[2]] > 0 and all(c[k] == 0 for k in W.COUNTS[3:])
    assert all(by_set["late_class"][k] == 0 for k in W.COUNTS)     # (its window is 140 bytes: what is late there is the haplotype)
    c = by_set["late_event_failure"]
    assert c[W.COUNTS[3]] == 4 * 3 + 4 and c[W.COUNTS[4]] == 8
    c = by_set["late_panic"]
    assert c[W.COUNTS[5]] == 4 * 3 + 8 + 3 and c[W.COUNTS[6]] == 16
    assert [by_set["many_regions_%d" % n][W.COUNTS[7]] for n in W.MANY] == [1, 1]
    assert [by_set["many_regions_%d" % n][W.COUNTS[8]] for n in W.MANY] == [0, 1]


def fates(set_name, name):
    return W.restated(set_name, name)["fates"]


def test_late_differences_are_what_they_claim():
    s = W.late_difference()
    for name, region in zip(s["names"], s["regions"]):
        r = W.restated("late_difference", name)
        assert r["status"] == 0 and r["new_padded"] == (W.RS + 30, W.RS + 669), name
        w = W.windows(region, r)
        assert all(len(x) == 640 for x in w), name
        if name.startswith("first_difference_at_"):
            k = int(name.rsplit("_", 1)[1])
            for a, b in ((0, 1), (0, 2), (1, 2)):
                assert [i for i in range(640) if w[a][i] != w[b][i]] == [k], (name, a, b)
            assert sorted(r["fates"]) == [0, 1, 2]
            for a, b in ((0, 1), (0, 2), (1, 2)):       # the order is that of the one byte
                assert (r["fates"][a] < r["fates"][b]) == (w[a][k] < w[b][k]), (name, a, b)
                order, t, q = W.model_compare(w[a], w[b])
                assert (t, q) == (k // 256, k % 256 // 64) and order == (-1 if w[a][k] < w[b][k] else 1)
    assert sorted({k // 256 for k in W.LATE_BYTES}) == [0, 1, 2] and sorted({k % 256 // 64 for k in W.LATE_BYTES}) == [0, 1, 2, 3]
    # two differences of opposite sign: byte 70 (A < G) decides against byte 200 (G > A), in either input order
    assert fates("late_difference", "opposite_signs_at_70_and_200") == [0, 1]
    assert fates("late_difference", "opposite_signs_at_70_and_200_reversed") == [1, 0]
    # byte 200 (T > G) decides; byte 300 (G < T) would have said the opposite
    assert fates("late_difference", "differences_at_200_and_300") == [1, 0]
    assert fates("late_difference", "differences_at_200_and_300_reversed") == [0, 1]
    r = W.restated("late_difference", "lower_case_folds_at_300")
    assert r["fates"] == [0, R.DUPLICATE, 1] and r["dup_of"] == [R.NONE32, 0, R.NONE32] and all(o[0] == o[0].upper() for o in r["out"])
    r = W.restated("late_difference", "lower_case_folds_at_300_lower_first")
    assert r["fates"] == [0, R.DUPLICATE] and r["out"][0][4] == 0 and r["out"][0][0][300:301] == b"C"
    region = s["regions"][s["names"].index("lower_case_folds_at_300_lower_first")]
    assert region[4][0][0][W.WINDOW0 + 300:W.WINDOW0 + 301] == b"c"


def test_witnesses_of_compare():
    """compare() cut to its first pass, and to three ballots of its first pass: the late pairs come out equal, and fold"""
    s = W.late_difference()
    short_pass, short_ballot = [], []
    for name, region in zip(s["names"], s["regions"]):
        r = W.restated("late_difference", name)
        w = W.windows(region, r)
        if name.startswith("lower_case"):
            assert W.model_compare(w[0], w[1]) == (0, 2, None)        # equal: all three passes
            assert W.model_compare(region[4][0][0][30:670], region[4][1][0][30:670]) == (0, 2, None)     # (as the input spells them)
            continue
        full = W.model_compare(w[0], w[1])[0]
        assert full != 0 and (full < 0) == (r["fates"][0] < r["fates"][1]), name
        if W.model_compare(w[0], w[1], passes=1)[0] != full:
            short_pass.append(name)
        if W.model_compare(w[0], w[1], ballots=3)[0] != full:
            short_ballot.append(name)
    assert short_pass == ["first_difference_at_%d" % k for k in (256, 257, 319, 320, 511, 512, 639)]
    assert short_ballot == ["first_difference_at_%d" % k for k in (192, 255, 511)] + [
        "differences_at_200_and_300", "differences_at_200_and_300_reversed"]
    # where only byte 200 is missed, byte 300 gives the opposite order
    for name in ("differences_at_200_and_300", "differences_at_200_and_300_reversed"):
        region = s["regions"][s["names"].index(name)]
        w = W.windows(region, W.restated("late_difference", name))
        assert W.model_compare(w[0], w[1], ballots=3)[0] == -W.model_compare(w[0], w[1])[0]


def test_a_class_with_members_in_three_trips():
    s = W.late_class()
    for name, region in zip(s["names"], s["regions"]):
        r = W.restated("late_class", name)
        refs = W.CLASS_REFS[name]
        rep = refs[-1] if refs else W.CLASS_AT[0]       # the last equal reference haplotype replaces key and value, else the first stays
        assert r["status"] == 0 and len(region[4]) == 301 and len(r["out"]) == 299, name
        assert [i for i, f in enumerate(r["fates"]) if f == R.DUPLICATE] == [i for i in W.CLASS_AT if i != rep], name
        assert all(r["dup_of"][i] == rep for i in W.CLASS_AT if i != rep) and r["fates"][rep] >= 0, name
        assert r["ref_hap"] == (r["fates"][rep] if refs else -1), name
        w = W.windows(region, r)
        assert len({bytes(x) for x in w}) == 299 and w[3] == w[70] == w[300] and len(w[0]) == 140


def test_witnesses_of_the_first_failure():
    """a search of one trip finds no failure behind haplotype 63: the region would have status 0, or the later one's status"""
    s = W.late_event_failure()
    _, _, event, panic = W.edge_parts()
    code = dict(ALLELES=EV.ALLELES, BAD_OPERATOR=EV.BAD_OPERATOR, BLOCK=EV.BLOCK, CIGAR_OVERRUN=EV.CIGAR_OVERRUN, LENGTH=R.LENGTH,
                LOCATION=R.LOCATION, OPERATOR=R.OPERATOR, NOT_FOUND=R.NOT_FOUND, REF_ELIMINATED=R.REF_ELIMINATED)
    for name, region in zip(s["names"], s["regions"]):
        r = W.restated("late_event_failure", name)
        assert r["fates"] == [R.NOT_TRIMMED] * 131 or name.startswith("healthy"), name
        if name.startswith("healthy"):
            assert r["status"] == 0 and len(r["out"]) == 2
            continue
        st = W.event_statuses(region)
        parts = name.split("_at_")                       # FAMILY_at_I or FAMILY_at_I_OTHER_at_J
        first = int(parts[1].split("_")[0])
        assert r["status"] == code[parts[0]] == st[first] and W.model_first([x < 0 for x in st]) == first, name
        one = W.model_first([x < 0 for x in st], trips=1)
        assert (one is None) == (first >= 64) and (first < 64 or r["status"] != 0), name
    s = W.late_panic()
    for name, region in zip(s["names"], s["regions"]):
        r = W.restated("late_panic", name)
        if name.startswith("healthy"):
            assert r["status"] == 0 and len(r["out"]) == 2
            continue
        st = W.panic_statuses(region, r)
        parts = name.split("_at_")
        first = int(parts[1].split("_")[0])
        assert r["status"] == code[parts[0]] == st[first] and W.model_first([x < 0 for x in st]) == first, name
        assert r["fates"] == [R.NOT_TRIMMED] * 260 and r["out"] == [] and r["ref_hap"] == -1, name
        assert (W.model_first([x < 0 for x in st], trips=1) is None) == (first >= 64), name
        if len(parts) == 3:          # two panics of different families: the later one's status is another
            second = int(parts[2])
            assert st[second] < 0 and st[second] != st[first] and second > first, name
    assert W.restated("late_panic", "LENGTH_at_129_REF_ELIMINATED_at_130")["status"] == R.LENGTH
    assert W.restated("late_panic", "REF_ELIMINATED_at_129_LENGTH_at_130")["status"] == R.REF_ELIMINATED


def test_witnesses_of_the_region_scan():
    for n in W.MANY:
        s = W.many_regions(n)
        rs = W.restated_regions("many_regions_%d" % n)
        n_out = [len(r["out"]) for r in rs]
        assert len(s["regions"]) == n and sorted(set(n_out)) == [0, 2, 3]
        assert all(not r["variation"] for r in rs[4::5]) and all(R.DUPLICATE in r["fates"] for g, r in enumerate(rs) if g % 11 == 0 and g % 5 != 4)
        want = R.trim_batch(s["regions"], s["dist"], s["padding"])["out_region_hap_off"]
        off, total = W.model_scan(n_out)
        assert off == want
        off, total = W.model_scan(n_out, chunk=1)
        assert off[:1024] == want[:1024] and off[1024:n] == [None] * (n - 1024)      # never written
        assert (total != want[n]) == any(n_out[1024:]) and (n == 1025 or any(n_out[1024:]))
    assert -(-2049 // 1024) == 3 and 683 * 3 == 2049     # three regions a thread, thread 683 and those behind it have none
