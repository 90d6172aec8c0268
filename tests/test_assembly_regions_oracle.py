"""CPU: holds tests/assembly_regions_restatement.py to the reference's own tests of pop_ready_assembly_regions
(tests/golden/assembly_region_cases.json: the grids and expected sizes of make_active_region_cut_tests, the properties of
region_creation_tests), to one hand-derived expectation per quirk, checks that header, ctypes module, wrapper and library
agree, and counts what the GPU case set reaches."""
import json
import os
import re

import numpy as np
import pytest

import assembly_regions_cases as K
import assembly_regions_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "assembly_region_cases.json")))
THRESHOLD, PROPAGATION, CONTIG = GOLDEN["active_prob_threshold"], GOLDEN["max_prob_propagation"], GOLDEN["contig_length"]
F32 = np.float32


def pop(probs, start=0, stop=None, contig=CONTIG, extension=0, mn=1, mx=300, prop=PROPAGATION, threshold=THRESHOLD):
    probs = list(probs)
    stop = start + len(probs) - 1 if stop is None else stop
    return R.Profile(probs, start, stop, contig, threshold, prop).pop_ready_assembly_regions(extension, mn, mx)


def spans(regions):
    return [(r["start"], r["end"]) for r in regions]


# ---- the layers agree ---------------------------------------------------------------------------------------------------------------
def test_the_module_the_header_and_the_restatement_name_the_same_values():
    import importlib
    from lorikeet_amd import _lib
    W = importlib.import_module("lorikeet_amd.assembly_regions")   # (the package exports the function under the module's name)
    header = open(os.path.join(ROOT, "include", "phmm.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"#define PHMM_REG_(\w+) \(?(-?\d+)u?\)?", header)}
    assert defines == dict(ACTIVE=1, FORCED=2, OVER_DEPTH=4, STATUS_MIN_REGION_SIZE=-1, STATUS_START_PAST_CONTIG=-2)
    internal = open(os.path.join(ROOT, "lorikeet_amd", "csrc", "phmm_regions_internal.hpp")).read()
    for name, value in defines.items():
        assert getattr(W, name) == value and getattr(R, name) == value and getattr(_lib, "PHMM_REG_" + name) == value, name
        assert re.search(r"REG_%s = %d\b" % (name, value), internal), name
    proto = re.search(r"int phmm_assembly_regions\((.*?)\);", header, re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in proto.split(",")]
    sym = [s for s in _lib.SYMBOLS if s[0] == "phmm_assembly_regions"]
    assert len(sym) == 1 and len(sym[0][2]) == len(names) == 39
    # the wrapper passes its arrays in the header's order, under the header's names
    assert [n for n, _ in W.PROFILE_INPUTS + W.READ_INPUTS] == names[11:24]
    assert ["capacity", "required"] + [n for n, _ in W.OUTPUTS] == names[24:]
    assert "float" not in re.sub(r"/\*.*?\*/", "", header, flags=re.S)   # f32 arrays travel as void pointers


def test_the_library_carries_the_regions_family_hash_and_the_layers_bind_the_export():
    from lorikeet_amd import _lib
    import lorikeet_amd
    import tools.source_hash as SH
    lib = _lib.load()
    assert "regions" in SH.KERNEL_SOURCES and "phmm_regions_kernels.hip" in SH.KERNEL_SOURCES["regions"]
    assert "regions=%s" % SH.source_hash("regions") in lib.phmm_build_info().decode()
    import importlib
    assert lorikeet_amd.assembly_regions is importlib.import_module("lorikeet_amd.assembly_regions").assembly_regions
    ffi = open(os.path.join(ROOT, "integration", "hip_ffi.rs")).read()
    backend = open(os.path.join(ROOT, "integration", "hip_backend.rs")).read()
    assert "pub fn phmm_assembly_regions(" in ffi
    assert "pub fn assembly_regions(" in backend and "phmm_assembly_regions(" in backend


# ---- the reference's own tests: make_active_region_cut_tests ----------------------------------------------------------------------------
def first_region_size(probs, mn, mx):
    """test_active_region_cuts (:572-608): states 0..=max + propagation, the probabilities then zeros; the first region's size."""
    n = mx + PROPAGATION + 1
    regions, status = pop([probs[i] if i < len(probs) else 0.0 for i in range(n)], mn=mn, mx=mx)
    assert status == 0 and len(regions) >= 1 and regions[0]["start"] == 0
    return regions[0]["end"] - regions[0]["start"] + 1


GRIDS = GOLDEN["cut_grids"]


def test_the_grid_is_the_references():
    assert [(g["size"], g["min_region_size"]) for g in GRIDS] == [(s, m) for s in (10, 12, 20, 30, 40) for m in (1, 5, 10) if m < s * 2 // 3]
    assert all(g["max_region_size"] == g["size"] * 2 // 3 for g in GRIDS)
    assert sum(len(g["two_peaks"]) for g in GRIDS) == 19


@pytest.mark.parametrize("shape", ["flat", "point", "increasing", "decreasing", "two_peaks"])
def test_the_cut_of_the_references_shapes(shape):
    for g in GRIDS:
        size, mn, mx = g["size"], g["min_region_size"], g["max_region_size"]
        if shape == "flat":
            cases = [([1.0] * size, g["flat"])]
        elif shape == "point":
            assert len(g["point"]) == size - 1
            cases = [([1.0] * end, g["point"][end - 1]) for end in range(1, size)]
        elif shape == "two_peaks":
            cases = [(c["probs"], c["expected"]) for c in g["two_peaks"]]
        else:
            assert len(g[shape]["probs"]) == size
            cases = [(g[shape]["probs"], g[shape]["expected"])]
        for probs, expected in cases:
            assert first_region_size(probs, mn, mx) == expected, (shape, size, mn, mx, probs)


def test_the_lowest_of_two_minima():
    """The reference computes these expectations and prints them; the call that would assert them is commented out
    (:775-781).  They are the original's, whose loop runs down to index min_region_size - 1 (a region of exactly the minimum
    size); the reference's loop is `while i >= min_region_size` (activity_profile.rs:592) and does not look at that index.  So
    the expectation holds wherever no minimum sits at index min_region_size - 1, and where one does the region is what the
    loop as written gives: the lowest eligible minimum in [min_region_size, max_region_size), else the maximum."""
    n_cases = differing = 0
    for g in GRIDS:
        size, mn, mx = g["size"], g["min_region_size"], g["max_region_size"]
        assert [len(row) for row in g["two_minima"]] == [size - 1 - first for first in range(1, size)]
        for first in range(1, size):
            for second in range(first + 1, size):
                expected = g["two_minima"][first - 1][second - first - 1]
                probs = [1.0] * size
                probs[first], probs[second] = 0.5, 0.75
                got = first_region_size(probs, mn, mx)
                # as written: 0.5 wins where the loop sees it; 0.75 is a minimum only when 0.5 is not its left neighbour
                if mn <= first <= mx - 1:
                    by_hand = first + 1
                elif mn <= second <= mx - 1 and second != first + 1:
                    by_hand = second + 1
                else:
                    by_hand = mx
                assert got == by_hand, (size, mn, mx, first, second)
                at_the_bound = first == mn - 1 or (first < mn - 1 and second == mn - 1 and second != first + 1)
                assert (got != expected) == at_the_bound, (size, mn, mx, first, second, got, expected)
                differing += got != expected
                n_cases += 1
    assert (n_cases, differing) == (4136, 178)


# ---- the reference's own tests: region_creation_tests ---------------------------------------------------------------------------------
def make_regions(total, start_with_active, n_parts):
    """make_regions (:262-278) as its comment describes it: parts of alternating activity.  As written its inner loop leaves at
    `j + i < total_region_size` (:269-271), which holds at once, so the reference's own lists are empty and its test holds
    vacuously; the properties are checked here on the lists it meant."""
    out, active, part = [], start_with_active, max(total // n_parts, 1)
    for i in range(0, total, part):
        out += [active] * min(part, total - i)
        active = not active
    return out


def test_the_properties_of_region_creation():
    g = GOLDEN["region_creation"]
    assert g["starts"][3:] == [CONTIG - 100, CONTIG - 10] and g["min_region_size"] == 1 and g["extension"] == 0
    n_cases = 0
    for start in g["starts"]:
        for size in g["sizes"]:
            size = min(size, CONTIG - start)
            for mx in g["max_region_sizes"]:
                for active_first in g["start_with_active"]:
                    for parts in g["parts"]:
                        probs = make_regions(size, active_first, parts)
                        regions, status = pop([1.0 if p else 0.0 for p in probs], start=start, mn=1, mx=mx)
                        assert status == 0
                        seen, last = [False] * len(probs), None
                        for r in regions:       # assert_good_regions (:348-403)
                            n = r["end"] - r["start"] + 1
                            assert 0 < n <= mx
                            assert last is None or r["start"] == last["end"] + 1
                            at = r["start"] - start
                            assert at < len(probs)
                            for j in range(n):
                                assert bool(r["flags"] & R.ACTIVE) == probs[at + j] and not seen[at + j]
                                seen[at + j] = True
                            last = r
                        # :338-345.  force_conversion is ignored as an argument (activity_profile.rs:376, :384-392): every
                        # region behind the first is popped under force, so either the list reaches max + propagation and
                        # every site is seen, or no region is made at all
                        assert all(seen) if len(probs) >= mx + PROPAGATION else not any(seen)
                        for i in range(len(probs)):
                            if i + mx + PROPAGATION < len(probs):
                                assert seen[i]
                        n_cases += 1
    assert n_cases == 5 * 5 * 3 * 2 * 9


# ---- one hand-derived expectation per quirk -----------------------------------------------------------------------------------------
def test_a_list_shorter_than_max_plus_propagation_yields_nothing():
    assert pop([1.0] * 20 + [0.0] * 39, mx=40, prop=20) == ([], 0)
    regions, _ = pop([1.0] * 20 + [0.0] * 40, mx=40, prop=20)
    assert spans(regions) == [(0, 19), (20, 59)]
    assert [r["flags"] for r in regions] == [R.ACTIVE, R.FORCED]      # the second is popped under force, 20 states before the end


def test_force_is_the_start_of_the_region_before_against_stop_plus_1():
    # 20 states from 100, the last ADDED one at 109: the third region starts at 110 = stop + 1, so the fourth try is unforced,
    # five states are fewer than 5 + 5, and the tail 115..119 stays unpopped
    regions, status = pop([0.0] * 20, start=100, stop=109, mx=5, prop=5)
    assert spans(regions) == [(100, 104), (105, 109), (110, 114)] and status == 0
    assert [r["flags"] for r in regions] == [0, R.FORCED, R.FORCED]
    regions, _ = pop([0.0] * 20, start=100, stop=110, mx=5, prop=5)
    assert spans(regions) == [(100, 104), (105, 109), (110, 114), (115, 119)]


def test_a_nan_is_inactive_and_the_threshold_is_strict():
    regions, _ = pop([1.0, 1.0, float("nan"), 1.0] + [1.0] * 6, mx=5, prop=5)
    assert spans(regions)[:3] == [(0, 1), (2, 2), (3, 7)] and [r["flags"] & 1 for r in regions[:3]] == [1, 0, 1]
    regions, _ = pop([F32(0.002)] * 4 + [F32(0.0020000001)] * 6 + [F32(0.0021)] * 2, mx=6, prop=6)   # 0.0020000001 as f32 is the threshold
    assert spans(regions)[0] == (0, 5) and not regions[0]["flags"] & 1


def test_the_cut_site_by_hand():
    base = [1.0] * 40 + [0.0] * 60
    def first(edits, mn=5, mx=30):  # noqa: E306
        p = list(base)
        for i, v in edits.items():
            p[i] = v
        regions, status = pop(p, mn=mn, mx=mx, prop=10)
        return regions[0]["states"] if regions else status
    assert first({}) == 30                                   # nothing qualifies: the end
    assert first({12: 0.5, 20: 0.25, 25: 0.75}) == 21        # the smallest probability
    assert first({12: 0.5, 20: 0.5}) == 21                   # equal values: the highest index, found first on the way down
    assert first({5: 0.5}) == 6 and first({4: 0.5}) == 30    # index min_region_size is looked at, the one below is not
    assert first({29: 0.5}) == 30                            # p[29] <= p[30] fails against the inactive 0.0 behind the run
    assert first({12: 0.5, 13: 0.5}) == 13                   # of a plateau only the first is < its left neighbour
    assert first({}, mn=31) == R.STATUS_MIN_REGION_SIZE      # the assertion, reached
    assert first({10: 0.0}, mn=31) == 10                     # ... and not reached: the run ends before the maximum


def test_is_minimum_is_of_the_current_list():
    # the last state of the whole list is no minimum: 20 states, max 20, the cut scans from index 19
    regions, _ = pop([1.0] * 18 + [0.75, 0.5], mn=1, mx=20, prop=0)
    assert regions[0]["states"] == 20
    # after [0, 6] is drained, index 0 of the remaining list holds a minimum of the whole list; the loop starts at
    # min_region_size >= 1 and never asks for it, and index 1 compares with it as its left neighbour
    p = R.Profile([0.0] * 7 + [1.0, 0.25, 0.5] + [1.0] * 30 + [0.0] * 40, 0, 79, CONTIG, THRESHOLD, 10)
    regions, _ = p.pop_ready_assembly_regions(0, 1, 10)
    assert spans(regions)[:2] == [(0, 6), (7, 8)]
    q = R.Profile([0.25, 0.5, 1.0], 0, 2, CONTIG, THRESHOLD, 0)
    assert not q.is_minimum(0) and not q.is_minimum(2) and not q.is_minimum(1)


def test_the_end_is_clipped_and_the_drained_states_are_not():
    # states at 10..20 on a contig of 20: the list keeps the state AT the contig length
    regions, status = pop([0.06] * 11, start=10, stop=19, contig=20, mx=4, prop=0)
    assert status == 0 and spans(regions) == [(10, 13), (14, 17), (18, 19)]
    assert [r["states"] for r in regions] == [4, 4, 3]
    assert regions[2]["density"] == F32(3) / F32(2)          # three drained states above 0.05 over a span of two
    assert pop([0.05] * 8, mx=4, prop=0)[0][0]["density"] == 0.0   # > 0.05, strictly


def test_a_region_that_starts_past_the_contig_ends_its_profile():
    regions, status = pop([0.0] * 10 + [1.0], start=10, stop=19, contig=20, mx=4, prop=0)
    assert status == R.STATUS_START_PAST_CONTIG and spans(regions) == [(10, 13), (14, 17), (18, 19)]


def test_the_padded_span_by_hand():
    assert R.make_padded_span(5, 14, 7, 100) == (0, 21)      # saturating
    assert R.make_padded_span(7, 16, 7, 100) == (0, 23)
    assert R.make_padded_span(90, 99, 7, 100) == (83, 100)   # min(contig LENGTH, end + padding): one past the last base
    assert R.make_padded_span(90, 99, 0, 100) == (90, 99)


def test_inactive_regions_are_returned_too():
    regions, _ = pop([0.0] * 30 + [1.0] * 30, mx=30, prop=30)
    assert [(r["flags"] & 1) for r in regions] == [0, 1] and spans(regions) == [(0, 29), (30, 59)]


def test_the_fetch_rule_and_the_depth_key_by_hand():
    # htslib: pos <= padded end && pos + max(reflen, 1) > padded start
    assert not R.fetched(980, 10, 990, 1059) and R.fetched(980, 11, 990, 1059)
    assert not R.fetched(989, 0, 990, 1059) and R.fetched(990, 0, 990, 1059)     # a read without reference bases counts as one
    assert R.fetched(1059, 1, 990, 1059) and not R.fetched(1060, 1, 990, 1059)
    enc = lambda *els: [(n << 4) | op for op, n in els]  # noqa: E731
    assert R.reference_length(enc((K.S, 5), (K.M, 5), (K.I, 3), (K.D, 1), (K.N, 7), (K.EQ, 2), (K.X, 1), (K.H, 9), (K.P, 4))) == 16
    assert R.mean_quality([10, 20, 40]) == np.float64(70.0) / np.float64(3.0)
    assert np.isnan(R.mean_quality([]))
    a, p = K.read_cases()["depth_above_cap"]
    o = run(a, p)
    assert list(o["region_n_reads"]) == [6] and o["region_flags"][0] == R.ACTIVE | R.OVER_DEPTH
    a, p = K.read_cases()["depth_at_cap"]
    assert run(a, p)["region_flags"][0] == R.ACTIVE          # records.len() > max_input_depth, strictly
    a, p = K.read_cases()["fetch_edges"]
    o = run(a, p)
    assert list(o["region_reads"]) == [1, 2, 4, 5, 6, 7] and np.isnan(run(*K.read_cases()["no_qualities"])["read_mean_qual"][0])


def run(a, p, branches=None, **kw):
    return R.assembly_regions(a, p["extension"], p["min_region_size"], p["max_region_size"], p["max_prob_propagation"], p["threshold"],
                              p["max_input_depth"], branches=branches, **kw)


# ---- what the GPU case set reaches ----------------------------------------------------------------------------------------------------
def test_census_of_the_gpu_case_set():
    reached = set()
    for name, (a, p) in K.all_cases().items():
        run(a, p, reached)
    assert K.CENSUS <= reached, sorted(K.CENSUS - reached)
    # index 0 of the remaining list is never asked for: the loop stops at min_region_size >= 1 (the one-line test above)
    assert "is_minimum:first" not in reached
    assert reached - K.CENSUS == set(), sorted(reached - K.CENSUS)
