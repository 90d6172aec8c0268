"""What tests/test_assembly_regions_wave_hip.py crosses, counted on the CPU from the inputs and the restatement alone
(tests/assembly_regions_wave_cases.py): second and later trips of the 64-lane loops of regions_cut_kernel, regions_span_kernel,
regions_read_kernel and regions_members_kernel, scans of more than one entry a thread, positions past 2^32.  Every count is above
0 on the new cases and 0 on assembly_regions_cases.all_cases() but for the three it reaches already (W.ALREADY); the loops as
restated in the case module give the restated result with their switches as they are, and each witness is a case whose restated
result a loop that stopped after its first trip, a scan of one entry a thread, a search without the last word's mask or a
position of 32 bits could not have given.  The restated loop headers are read out of the source text: when one is rewritten, the
case list needs another look.  No GPU."""
import os
import re
import time

import numpy as np
import pytest

import assembly_regions_cases as K
import assembly_regions_wave_cases as W
from conftest import ROOT

CSRC = os.path.join(ROOT, "lorikeet_amd", "csrc")
NEW = sorted(W.CASES)


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_restated_loops_are_the_sources():
    kernels, internal = _source("phmm_regions_kernels.hip"), _source("phmm_regions_internal.hpp")
    m = re.search(r"constexpr\s+uint32_t\s+REG_SCAN_THREADS\s*=\s*(\d+)u?\s*;", internal)
    assert m and int(m.group(1)) == W.SCAN_THREADS == 1024
    for kernel in ("regions_cut_kernel", "regions_span_kernel", "regions_pmax_kernel", "regions_count_kernel", "regions_members_kernel"):
        assert "__launch_bounds__(64) void %s" % kernel in kernels, kernel
    once = ("for (uint32_t base = w0; base <= w1; base += 64) {",
            "if (w == w0) x &= ~bits_below(cur & 63u);",
            "if (w == w1) x &= bits_below(((cur + limit - 1) & 63u) + 1);",
            "for (uint32_t i = p.min_size + lane; i < e; i += 64) {",
            "const uint32_t per = (n + REG_SCAN_THREADS - 1) / REG_SCAN_THREADS;  // a run of `per` entries a thread",
            "const uint32_t b = t * per < n ? t * per : n, e = b + per < n ? b + per : n;",
            "for (uint32_t w = w0 + lane; w <= w1; w += 64) {",
            "if (w == w0) x &= ~bits_below(first & 63u);",
            "if (w == w1) x &= bits_below(((first + n - 1) & 63u) + 1);",
            "for (uint32_t c = p.cigar_off[r] + lane; c < p.cigar_off[r + 1]; c += 64) {",
            "for (uint32_t b = b0 + lane; b < b1; b += 64) qsum += p.quals[b];",
            "for (uint32_t base = r0; base < r1; base += 64) {",
            "const uint32_t r = blockIdx.x * 64 + threadIdx.x;")
    for line in once:
        assert kernels.count(line) == 1, line
    assert kernels.count("for (uint32_t base = lo; base < hi; base += 64) {") == 2     # the count, then the members
    assert kernels.count("regions_block_scan(") == 3                                  # the definition, profiles, pairs


def add(total, c):
    for k, v in c.items():
        total[k] += v


def test_census_of_the_wave_cases_and_of_the_first_suite():
    t0 = time.perf_counter()
    total = dict.fromkeys(W.COUNTS, 0)
    by_case = {}
    for name in NEW:
        a, p = W.case(name)
        by_case[name] = W.census(a, p, W.restated(name))
        add(total, by_case[name])
    print("\nthe wave cases of phmm_assembly_regions: %d calls, restated in %.1f s" % (len(NEW), time.perf_counter() - t0))
    for k in W.COUNTS:
        print("  %-82s %6d" % (k, total[k]))
        assert total[k] > 0, k
    old = dict.fromkeys(W.COUNTS, 0)
    old_by_case = {}
    for name, (a, p) in K.all_cases().items():
        old_by_case[name] = W.census(a, p, W.restate(a, p))
        add(old, old_by_case[name])
    for k in W.COUNTS:
        assert old[k] == W.ALREADY.get(k, 0), (k, old[k])
    # the three the first suite reaches, by name
    assert old_by_case["boundary_word70"][W.COUNTS[3]] == 1 and old_by_case["boundary_word70"][W.COUNTS[4]] == 0
    assert old_by_case["boundary_word70"][W.COUNTS[5]] == 1 and old_by_case["boundary_word70"][W.COUNTS[6]] == 0
    assert old_by_case["two_windows"][W.COUNTS[14]] == 1
    # each family is there for counts of its own
    for n in W.SCAN_SIZES:
        assert by_case["scan_profiles_%d" % n][W.COUNTS[0]] == (n > 1024) and by_case["scan_pairs_%d" % n][W.COUNTS[1]] == (n > 1024)
    assert by_case["scan_profiles_2049"][W.COUNTS[2]] == 1 and by_case["scan_pairs_2049"][W.COUNTS[2]] == 1
    assert by_case["together"][W.COUNTS[1]] == 1 and by_case["together"][W.COUNTS[14]] >= 3 and by_case["together"][W.COUNTS[16]] > 0
    for n in W.SPAN_SIZES:
        for f in W.SPAN_FIRST:
            for kind in ("dense", "sparse"):
                c = by_case["span_%s_%d_first%d" % (kind, n, f)]
                two = (f + n - 1) >> 6 >= 64      # (4096 states from index 0 are 64 words: one trip of the popcount)
                assert c[W.COUNTS[3]] == c[W.COUNTS[4]] == two and c[W.COUNTS[5]] >= 1, (kind, n, f)
                assert c[W.COUNTS[6]] == (kind == "dense") and c[W.COUNTS[7]] == (f > 0), (kind, n, f)
    assert all(by_case["cut_inactive_%d_lead%d" % (n, lead)][W.COUNTS[8]] == 1 for n in (4100, 4101, 4102, 4300) for lead in (0, 37))
    assert all(by_case["cut_%s_lead%d" % (k, lead)][W.COUNTS[9]] == 1 for k in ("inactive_4101", "inactive_4102", "active_4102") for lead in (0, 37))
    assert by_case["cut_site_equal_4096_apart"][W.COUNTS[11]] == 1 and by_case["cut_site_none_min_size_1"][W.COUNTS[11]] == 1
    assert by_case["cut_site_one_minimum_4090"][W.COUNTS[10]] == 1 and by_case["cut_site_one_minimum_4090"][W.COUNTS[11]] == 0
    assert [by_case["cigar_%d_elements" % n][W.COUNTS[12]] for n in W.CIGAR_SIZES] == [0, 0, 1, 2]
    assert by_case["cigar_130_elements"][W.COUNTS[13]] == 2
    assert [by_case["members_%d" % n][W.COUNTS[14]] for n in W.MEMBER_SIZES] == [0, 0, 1, 2, 2]
    assert [by_case["members_%d" % n][W.COUNTS[15]] for n in W.MEMBER_SIZES] == [0, 0, 0, 0, 1]


def spans_of(a, want):
    """per region: (profile, group of sample 0, padded start, padded end)"""
    S = int(a["n_samples"])
    for r, k, _, _, _ in W.regions_of(a, want):
        yield r, k, int(a["profile_window"][k]) * S, int(want["region_padded_start"][r]), int(want["region_padded_end"][r])


@pytest.mark.parametrize("name", NEW)
def test_the_restated_loops_give_the_restated_result(name):
    """the models of the case module with every switch as the kernels have it: states, density, offsets, reads"""
    a, p = W.case(name)
    want = W.restated(name)
    assert not want["profile_status"].any()
    kept = {}
    for r, k, cur, e, flags in W.regions_of(a, want):
        if k not in kept:
            kept[k] = W.planes(a, p, k)
        active, dense, q = kept[k]
        limit = min(len(active) - cur, p["max_region_size"])
        found, _ = W.model_boundary(active, cur, limit)
        if active[cur] and found == p["max_region_size"]:
            found = W.model_cut_site(q, cur, found, p["min_region_size"])
        assert found == e and bool(active[cur]) == bool(flags & 1), (r, found, e)
        size = int(want["region_end"][r]) - int(want["region_start"][r]) + 1
        assert W.model_density(dense, cur, e, size) == want["region_density"][r], r
    counts = np.diff(np.asarray(want["profile_region_off"], np.int64))
    off, total = W.model_scan(counts)
    assert off == list(want["profile_region_off"]) and total == want["required"][0]
    if a.get("group_read_off") is None:
        return
    off, total = W.model_scan(np.diff(np.asarray(want["region_read_off"], np.int64)))
    assert off == list(want["region_read_off"]) and total == want["required"][1]
    ends = W.read_ends(a)
    members = []
    for r, k, g0, ps, pe in spans_of(a, want):
        for s in range(int(a["n_samples"])):
            members += W.model_members(a, ends, g0 + s, ps, pe)
    assert members == list(want["region_reads"])
    for r in range(len(ends)):
        quals = a["read_quals"][a["read_off"][r]:a["read_off"][r + 1]]
        if len(quals):
            assert np.float64(W.model_qsum(quals)) / np.float64(len(quals)) == want["read_mean_qual"][r], r


def test_the_case_shapes_are_what_they_claim():
    for n in W.SCAN_SIZES:
        a, _ = W.case("scan_profiles_%d" % n)
        want = W.restated("scan_profiles_%d" % n)
        counts = np.diff(np.asarray(want["profile_region_off"], np.int64))
        assert len(a["profile_len"]) == n and sorted(set(counts)) == [0, 1, 2, 3] and not a["profile_len"][3::7].any() and a["profile_len"].max() == 12
    for n, (regions, samples) in W.PAIR_SHAPES.items():
        want = W.restated("scan_pairs_%d" % n)
        per_pair = np.diff(np.asarray(want["region_read_off"], np.int64))
        assert want["required"][0] == regions and len(per_pair) == n == regions * samples
        assert sorted(set(want["region_states"])) == [2, 3] and list(want["region_states"]).count(2) == 2
        assert len(set(per_pair)) >= 4 and np.count_nonzero(per_pair) > n // 2 and np.count_nonzero(per_pair == 0) > n // 20, (n, np.bincount(per_pair))
    for n in W.SPAN_SIZES:
        for f in W.SPAN_FIRST:
            for kind in ("dense", "sparse"):
                name = "span_%s_%d_first%d" % (kind, n, f)
                (a, p), want = W.case(name), W.restated(name)
                r = 1 if f else 0
                assert want["region_states"][r] == n and want["region_start"][r] == 500 + f and bool(want["region_flags"][r] & 1) == (kind == "dense")
                assert 0.4 < want["region_density"][r] < 0.6
                _, dense, _ = W.planes(a, p, 0)
                for w in (64, (f + n - 1) >> 6):      # the word just past 64 words and the region's last hold both kinds
                    inside = dense[max(w * 64, f):min(w * 64 + 64, f + n)]
                    assert 0 < np.count_nonzero(inside) < len(inside) or len(inside) <= 1, (name, w)
                beside = np.count_nonzero(dense[:f]) + np.count_nonzero(dense[f + n:])
                assert beside == (f + 20 if kind == "sparse" else 0)
    for n in W.MEMBER_SIZES:
        a, _ = W.case("members_%d" % n)
        want = W.restated("members_%d" % n)
        assert list(np.diff(np.asarray(want["region_read_off"], np.int64))) == [n, n // 2 + 3]
        ends = W.read_ends(a)
        ps, pe = int(want["region_padded_start"][0]), int(want["region_padded_end"][0])
        for g, n_candidates in ((0, 200), (1, 150)):
            lo, hi = W.candidates(a, ends, g, ps, pe)
            assert hi - lo == n_candidates
            for base in range(lo, hi, 64):        # every pass of 64 candidates holds members and others
                inside = [ends[i] > ps for i in range(base, min(base + 64, hi))]
                assert any(inside) and not all(inside), (n, g, base)
    for n in W.CIGAR_SIZES:
        a, _ = W.case("cigar_%d_elements" % n)
        want = W.restated("cigar_%d_elements" % n)
        n_cigar = list(np.diff(np.asarray(a["read_cigar_off"], np.int64)))
        assert n_cigar[:2] == [n, n - 1] and {int(c) & 15 for c in a["read_cigar"][:n]} == set(range(9))
        reached = list(want["region_reads"])
        assert 0 in reached and 1 not in reached and (n <= 64 or 2 not in reached)
        lens = list(np.diff(np.asarray(a["read_off"], np.int64)))[-len(W.QUAL_LENGTHS):]
        assert lens == list(W.QUAL_LENGTHS) and 255 in a["read_quals"] and len(set(a["read_quals"])) > 50
    want = W.restated("positions_past_2_32")
    starts, ends = [int(x) for x in want["region_start"]], [int(x) for x in want["region_end"]]
    assert any(s < W.P32 <= e for s, e in zip(starts, ends)) 
    # an extension that reaches across 2^32 from a region that lies on one side of it
    assert any(int(s) < W.P32 <= x for s, x in zip(want["region_padded_start"], starts)) or any(x < W.P32 <= int(e) for e, x in zip(want["region_padded_end"], ends))
    assert ends[-1] == W.P62 - 2 and starts[-1] + int(want["region_states"][-1]) - 1 == W.P62 - 1      # clipped at the contig's end
    assert int(want["region_padded_end"][-1]) == W.P62 - 1 and want["region_n_reads"][-1] > 0
    assert np.count_nonzero(want["region_n_reads"][:int(want["profile_region_off"][1])]) >= 3


def region_index(name, active):
    want = W.restated(name)
    return [r for r in range(len(want["region_flags"])) if bool(want["region_flags"][r] & 1) == active][0]


def test_witnesses_of_the_boundary_search():
    """the boundary behind 64 words: a search of one trip gives `limit`; one without the last word's mask runs past max_region_size"""
    found_late = [("cut_active_4099_lead%d" % lead, True) for lead in (0, 37)] + [("cut_site_nan_4097_beside_200", True)]
    found_late += [("span_%s_%d_first%d" % (kind, n, f), kind == "dense") for kind in ("dense", "sparse") for n in W.SPAN_SIZES for f in W.SPAN_FIRST]
    for name, is_active in found_late:
        (a, p), want = W.case(name), W.restated(name)
        r = region_index(name, is_active)
        active, _, _ = W.planes(a, p, 0)
        cur, e = int(want["region_start"][r]) - int(a["profile_start"][0]), int(want["region_states"][r])
        limit = min(len(active) - cur, p["max_region_size"])
        assert W.model_boundary(active, cur, limit)[0] == e and W.model_boundary(active, cur, limit, trips=1)[0] == limit != e, name
    for name, is_active in [("cut_%s_lead%d" % (k, lead), k[0] == "a") for k in ("inactive_4101", "inactive_4102", "active_4102") for lead in (0, 37)]:
        (a, p), want = W.case(name), W.restated(name)
        r = region_index(name, is_active)
        active, _, _ = W.planes(a, p, 0)
        cur = int(want["region_start"][r]) - int(a["profile_start"][0])
        assert cur == int(name[-2:].replace("d", "")) and want["region_states"][r] == W.MAX_4100
        assert W.model_boundary(active, cur, W.MAX_4100)[0] == W.MAX_4100 != W.model_boundary(active, cur, W.MAX_4100, mask=False)[0], name
    # the run of 4102 is cut AT 4100 because the mask hides the boundary at 4102; 4099 and 4100 are whole
    for lead in (0, 37):
        assert [int(W.restated("cut_active_%d_lead%d" % (n, lead))["region_states"][1 if lead else 0]) for n in (4099, 4100, 4102)] == [4099, 4100, 4100]
        assert int(W.restated("cut_active_4102_lead%d" % lead)["region_states"][(1 if lead else 0) + 1]) == 2
    want = W.restated("cut_forced_tail_word65")
    assert list(want["region_states"]) == [100, 4090] and want["region_flags"][1] == 3 and (100 + 4090 - 1) >> 6 == 65


def test_witnesses_of_the_cut_site():
    expect = {"one_minimum_4090": 4091, "one_minimum_70": 71, "one_minimum_70_lead37": 71, "equal_100_and_4000": 4001, "equal_64_apart": 75,
              "equal_4096_apart": 4099, "lower_early_beats_equal_late": 10, "none": 4100, "none_min_size_1": 4100, "nan_4000_beside_200": 4000, "nan_4097_beside_200": 4097,
              "nan_behind_end": 201, "minimum_at_end_minus_1": 4100, "minimum_at_end": 4100}
    one_trip_differs = []
    for name, e in expect.items():
        (a, p), want = W.case("cut_site_" + name), W.restated("cut_site_" + name)
        r = region_index("cut_site_" + name, True)
        assert want["region_states"][r] == e, (name, want["region_states"][:4])
        if name.startswith("nan_40"):
            continue                     # (no cut site: the boundary)
        _, _, q = W.planes(a, p, 0)
        cur = int(want["region_start"][r]) - int(a["profile_start"][0])
        assert W.model_cut_site(q, cur, W.MAX_4100, p["min_region_size"]) == e
        if W.model_cut_site(q, cur, W.MAX_4100, p["min_region_size"], trips=1) != e:
            one_trip_differs.append(name)
    assert one_trip_differs == ["one_minimum_4090", "one_minimum_70", "one_minimum_70_lead37", "equal_100_and_4000", "equal_64_apart",
                                "equal_4096_apart", "nan_behind_end"]


def test_witnesses_of_the_density():
    for kind in ("dense", "sparse"):
        for n in W.SPAN_SIZES:
            for f in W.SPAN_FIRST:
                name = "span_%s_%d_first%d" % (kind, n, f)
                (a, p), want = W.case(name), W.restated(name)
                _, dense, _ = W.planes(a, p, 0)
                r = 1 if f else 0
                args = (dense, f, n, n)
                two = (f + n - 1) >> 6 >= 64      # (4096 states from index 0 are 64 words: one trip)
                assert W.model_density(*args) == want["region_density"][r] and (W.model_density(*args, trips=1) != want["region_density"][r]) == two, name
                # a popcount without the last word's mask counts the neighbours' bits, where the threshold lets them be set
                ends_inside_word = (f + n) % 64 != 0
                assert (W.model_density(*args, mask=False) != want["region_density"][r]) == (kind == "sparse" and ends_inside_word), name


def test_witnesses_of_the_scans():
    for family, key in (("scan_profiles_%d", "profile_region_off"), ("scan_pairs_%d", "region_read_off")):
        for n in W.SCAN_SIZES:
            want = W.restated(family % n)
            v = np.diff(np.asarray(want[key], np.int64))
            off, total = W.model_scan(v, per=1)
            if n <= 1024:
                assert off == list(want[key])
            else:
                assert off[:1024] == list(want[key][:1024]) and off[1024:n] == [None] * (n - 1024), (family, n)     # never written
                assert (total != want[key][n]) == bool(v[1024:].any()) and (n == 1025 or v[1024:].any()), (family, n)
    # 2049 entries: three a thread, thread 683 and those behind it have none
    assert -(-2049 // W.SCAN_THREADS) == 3 and 683 * 3 == 2049


def test_witnesses_of_the_reads():
    for n in (65, 130):
        name = "cigar_%d_elements" % n
        (a, _), want = W.case(name), W.restated(name)
        ps, pe = int(want["region_padded_start"][0]), int(want["region_padded_end"][0])
        assert W.model_members(a, W.read_ends(a), 0, ps, pe) == list(want["region_reads"])
        assert 0 not in W.model_members(a, W.read_ends(a, trips=1), 0, ps, pe)
        if n == 130:
            assert 0 not in W.model_members(a, W.read_ends(a, trips=2), 0, ps, pe)
    for n in W.MEMBER_SIZES:
        (a, _), want = W.case("members_%d" % n), W.restated("members_%d" % n)
        ps, pe = int(want["region_padded_start"][0]), int(want["region_padded_end"][0])
        ends = W.read_ends(a)
        full, one = W.model_members(a, ends, 0, ps, pe), W.model_members(a, ends, 0, ps, pe, trips=1)
        assert full == list(want["region_reads"][:n]) and one == full[:len(one)] and 0 < len(one) < n
    (a, _), want = W.case("cigar_130_elements"), W.restated("cigar_130_elements")
    for r in range(len(a["read_pos"])):
        quals = a["read_quals"][a["read_off"][r]:a["read_off"][r + 1]]
        if len(quals) > 64:
            assert np.float64(W.model_qsum(quals, trips=1)) / np.float64(len(quals)) != want["read_mean_qual"][r]


def test_witnesses_of_the_positions():
    """positions kept to 32 bits: the outputs lose their upper half, and the reads of a region that straddles 2^32 are others"""
    (a, _), want = W.case("positions_past_2_32"), W.restated("positions_past_2_32")
    m = (1 << 32) - 1
    for k in ("region_start", "region_end", "region_padded_start", "region_padded_end"):
        assert any(int(x) & m != int(x) for x in want[k]), k
    ends64, ends32 = W.read_ends(a), W.read_ends(a, bits=32)
    differ = 0
    for r, k, g0, ps, pe in spans_of(a, want):
        for s in range(int(a["n_samples"])):
            differ += W.model_members(a, ends64, g0 + s, ps, pe) != W.model_members(a, ends32, g0 + s, ps & m, pe & m, bits=32)
    assert differ >= 2
