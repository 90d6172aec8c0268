"""CPU checks around phmm_activity_profile: the restatement (tests/activity_restatement.py) held to the reference's own test
vectors and grids (tests/golden/activity_profile_cases.json, extracted by tests/golden/make_activity_profile_cases.py) and to
pileups worked by hand, the host-made C tables held to the restatement bit for bit, and a census of the cases
tests/test_activity_hip.py runs on the GPU, so that none of them is vacuous.  The module imports lorikeet_amd.activity at the
top: without the call every test here fails."""
import ctypes as C
import json
import math
import os
import re
from collections import Counter

import numpy as np
import pytest

import activity_cases as K
import activity_restatement as R
from conftest import GOLDEN, ROOT
from lorikeet_amd import _lib, activity  # noqa: F401

CASES = json.load(open(os.path.join(GOLDEN, "activity_profile_cases.json")))
F32 = np.float32


def approx_relative_eq(a, b, epsilon):
    """The approx crate's relative_eq!(a, b, epsilon = e) as the reference's tests call it: |a - b| <= e, or within the type's
    epsilon relative to the larger."""
    d = abs(float(a) - float(b))
    return d <= epsilon or d <= max(abs(float(a)), abs(float(b))) * float(np.finfo(np.float32).eps)


def c_kernel(max_size, sigma, adaptive=True):
    lib = _lib.load()
    fs = np.zeros(1, np.uint32)
    k = np.zeros(2 * max_size + 1)
    assert lib.phmm_activity_band_kernel(max_size, sigma, int(adaptive), fs.ctypes.data_as(_lib.u32p), k.ctypes.data_as(_lib.f64p)) == _lib.PHMM_OK
    return int(fs[0]), k[:2 * int(fs[0]) + 1]


def test_the_export_is_in_the_library_the_binding_and_the_rust_declarations():
    lib = _lib.load()
    names = ("phmm_activity_profile", "phmm_activity_band_kernel", "phmm_activity_term_table")
    ffi = open(os.path.join(ROOT, "integration", "hip_ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "phmm.h")).read()
    for n in names:
        assert getattr(lib, n) is not None
        assert n in {s[0] for s in _lib.SYMBOLS}
        assert re.search(r"pub fn %s\s*\(" % n, ffi), n
        assert re.search(r"\bint %s\(" % n, header), n
    args = next(a for n, _, a in _lib.SYMBOLS if n == "phmm_activity_profile")
    decl = re.search(r"pub fn phmm_activity_profile\s*\(([^)]*)\)", ffi, re.S).group(1)
    assert len(args) == len([x for x in decl.split(",") if x.strip()]) == 40
    import tools.source_hash as SH
    assert "phmm_activity_kernels.hip" in SH.KERNEL_SOURCES["activity"]
    assert "activity=%s" % SH.source_hash("activity") in lib.phmm_build_info().decode()


@pytest.mark.parametrize("case", CASES["kernel_creation"], ids=lambda c: "sigma%s-size%d" % (c["sigma"], c["max_size"]))
def test_kernel_creation_vectors(case):
    """make_kernel_creation: adaptive, at 1e-3 relative; and the C table equals the restatement's bit for bit."""
    prof = R.BandPassActivityProfile(CASES["max_prob_propagation_distance"], case["max_size"], case["sigma"], True, CASES["contig_len"])
    kernel = prof.gaussian_kernel
    assert len(kernel) == len(case["expected"])
    for got, want in zip(kernel, case["expected"]):
        assert abs(got - want) <= 1e-3 * max(abs(got), abs(want)), (got, want)
    fs, ck = c_kernel(case["max_size"], case["sigma"])
    assert fs == prof.filter_size and ck.tobytes() == np.array(kernel).tobytes()


def test_fixed_size_kernels_and_refused_sigmas():
    for size, sigma in ((0, 1.0), (1, 2.0), (12, 3.0), (50, 17.0), (100, 17.0)):
        fs, ck = c_kernel(size, sigma, adaptive=False)
        assert fs == size and ck.tobytes() == np.array(R.make_kernel(size, sigma)).tobytes()
    lib = _lib.load()
    fs = np.zeros(1, np.uint32)
    for sigma in (-1.0, 0.0, float("nan")):  # the reference's assertions: sd >= 0, a sum >= 0
        assert lib.phmm_activity_band_kernel(5, sigma, 1, fs.ctypes.data_as(_lib.u32p), None) == _lib.PHMM_ERR_INVALID_ARG


@pytest.mark.parametrize("ploidy", [1, 2, 3, 4, 64])
def test_term_table_equals_the_restatement(ploidy):
    t = np.zeros((2, 256, ploidy + 1))
    assert _lib.load().phmm_activity_term_table(ploidy, t.ctypes.data_as(_lib.f64p)) == _lib.PHMM_OK
    want = R.term_table(ploidy)
    assert t.tobytes() == want.tobytes(), np.argwhere(t != want)[:5]


def test_band_pass_grid():
    """make_band_pass_test: filter size and band size as given; the profile sums to the number of active states within 1e-3
    where the reference asserts it."""
    g = CASES["band_pass_test"]
    asserted = 0
    for start in g["start"]:
        for active in g["preceding_is_active"]:
            for n_pre in g["preceding_sites"]:
                for size in g["band_pass_size"]:
                    for sigma in g["sigma"]:
                        prof = R.BandPassActivityProfile(CASES["max_prob_propagation_distance"], size, sigma, False, CASES["contig_len"])
                        assert prof.filter_size == size and len(prof.gaussian_kernel) == 2 * size + 1
                        for i in range(n_pre):
                            prof.add(i + start, F32(1.0 if active else 0.0), None)
                        prof.add(n_pre + start, F32(1.0), None)
                        if not active and n_pre >= size and size < start:
                            total = F32(0.0)
                            for x in prof.state_list:
                                total = total + x
                            assert approx_relative_eq(total, 1.0, 1e-3), (start, n_pre, size, sigma, total)
                            asserted += 1
    assert asserted > 20


def band_pass_in_one_pass(prof, active):
    out = []
    fs, kern = prof.filter_size, prof.gaussian_kernel
    for i in range(len(active)):
        kernel = kern[max(fs - i, 0):min(len(kern), fs + len(active) - i)]
        sub = active[max(i - fs, 0):min(len(active), i + fs + 1)]
        s = 0.0
        for a, b in zip(sub, kernel):  # MathUtils::dot_product
            s += a * b
        out.append(F32(s))
    return out


def test_band_pass_composition():
    g = CASES["band_pass_composition"]
    for size in g["band_pass_size"]:
        for length in g["integration_length"]:
            prof = R.BandPassActivityProfile(CASES["max_prob_propagation_distance"], size, R.DEFAULT_SIGMA, True, CASES["contig_len"])
            raw = [0.0] * (length + size * 2)
            pos = 1
            for _ in range(size):
                prof.add(pos, F32(0.0), None)
                pos += 1
            for i in range(length):
                prof.add(pos, F32(1.0), None)
                pos += 1
                raw[size + i] = 1.0
            assert all(0.0 <= x <= 1.0 + 1e-3 for x in prof.state_list)
            want = band_pass_in_one_pass(prof, raw)
            for j, x in enumerate(prof.state_list):
                assert approx_relative_eq(x, want[j], 1e-3), (size, length, j, x, want[j])


def test_soft_clip_grid():
    """run_test_soft_clips (activity_profile_unit_tests.rs:451-533): the profile's size, and which states are positive."""
    g, L, reach = CASES["soft_clips"], CASES["contig_len"], CASES["max_prob_propagation_distance"]
    for start in g["start"]:
        start = L - int(start.split("-")[1]) if "-" in start else int(start)
        for n_pre in g["preceding_sites"]:
            if n_pre + start >= L:
                continue
            for clip in g["soft_clip_size"]:
                prof = R.ActivityProfile(reach, L)
                for i in range(n_pre):
                    prof.add(i + start, F32(0.0), None)
                at = n_pre + start
                prof.add(at, F32(1.0), F32(clip))
                actual = min(clip, reach)
                if n_pre == 0:
                    assert len(prof.state_list) == min(start + actual, L) - start + 1
                for i, x in enumerate(prof.state_list):
                    assert (x > 0.0) == (abs(start + i - at) <= actual), (start, n_pre, clip, i)


# ---- the pileup, by hand (the reference has no test of parse_record) -------------------------------------------------------------

REF = b"ACGTACGTACGTACGTACGT"
LOG3 = math.log10(3.0)


def pile(reads, ploidy, bq=10):
    lk, clips = R.update_activity_profile([[R.Record(*r) for r in reads]], REF, 100, len(REF), 10000, ploidy, bq)
    return lk[0], clips


@pytest.mark.parametrize("ploidy", [1, 2, 3])
def test_one_matching_read_in_closed_form(ploidy):
    lk, clips = pile([(105, "10M", REF[5:15], [30] * 10)], ploidy)
    right, wrong = math.log10(1.0 - 10.0 ** -3.0), 30 * -0.1 + -LOG3
    lp = math.log10(float(ploidy))
    for p, r in enumerate(lk):
        inside = 5 <= p < 15
        assert (r.read_counts, r.ref_depth, r.non_ref_depth) == ((1, 1, 0) if inside else (0, 0, 0))
        if not inside:
            assert r.genotype_likelihoods == [0.0] * (ploidy + 1)
            continue
        gl = r.genotype_likelihoods
        assert gl[0] == (0.0 + (right + lp)) - 1.0 * lp and gl[ploidy] == (0.0 + (wrong + lp)) - 1.0 * lp
        for i in range(1, ploidy):  # log10(j 10^right + i 10^wrong) - log10(ploidy), through the table: 1e-4 steps of the difference
            exact = math.log10((ploidy - i) * 10.0 ** right + i * 10.0 ** wrong) - lp
            assert abs(gl[i] - exact) < 1e-4, (i, gl[i], exact)
        assert clips[p].obs_count == 0
    assert abs(lk[5].genotype_likelihoods[0] - right) < 1e-15 and abs(lk[5].genotype_likelihoods[ploidy] - wrong) < 1e-15


def test_one_mismatch_one_deletion_one_low_quality_base():
    quals = [30] * 10
    quals[7] = 5  # below bq: not counted at all
    bases = bytearray(REF[5:15])
    bases[3] = ord("A") if bases[3] != ord("A") else ord("C")  # position 108
    lk, _ = pile([(105, "10M", bytes(bases), quals)], 2)
    right, wrong = math.log10(1.0 - 10.0 ** -3.0), 30 * -0.1 + -LOG3
    assert (lk[8].read_counts, lk[8].ref_depth, lk[8].non_ref_depth) == (1, 0, 1)
    assert abs(lk[8].genotype_likelihoods[0] - wrong) < 1e-15 and abs(lk[8].genotype_likelihoods[2] - right) < 1e-15
    assert (lk[12].read_counts, lk[12].ref_depth, lk[12].non_ref_depth) == (0, 0, 0) and lk[12].genotype_likelihoods == [0.0] * 3
    # a deletion: Q30, alt, counted whatever bq is; the bases beside it are alt too (next to an indel)
    lk, _ = pile([(102, "4M3D4M", REF[2:6] + REF[9:13], [40] * 8)], 2, bq=35)
    for p in (6, 7, 8):
        assert (lk[p].read_counts, lk[p].non_ref_depth) == (1, 1)
        assert abs(lk[p].genotype_likelihoods[0] - wrong) < 1e-15 and abs(lk[p].genotype_likelihoods[2] - right) < 1e-15
    assert [lk[p].non_ref_depth for p in (2, 3, 4, 5, 9, 10, 11, 12)] == [0, 0, 0, 1, 1, 0, 0, 0]


def test_soft_clip_average_in_order():
    """Two reads add 8 and 3 at the same position: the mean after each, one operation at a time."""
    a = (105, "8S10M", b"T" * 8 + REF[5:15], [40] * 18)
    b = (105, "3S10M", b"T" * 3 + REF[5:15], [29] * 13)
    _, clips = pile([a, b], 2)
    assert clips[5].obs_count == 2 and clips[5].mean() == 8.0 + (3.0 - 8.0) / 2.0
    _, clips = pile([b, a], 2)
    assert clips[5].mean() == 3.0 + (8.0 - 3.0) / 2.0 and clips[6].obs_count == 0


# ---- the census of the GPU cases ----------------------------------------------------------------------------------------------

def test_census_of_the_gpu_cases():
    total = Counter()
    seen = Counter()
    for name, windows, o in K.all_cases():
        r, trace = K.restated(name)
        total.update(trace)
        F, reach = r["filter_size"], o["max_prob_propagation"]
        # no tolerance may hide a different `qual as u8`: QUAL stays clear of every integer in 1..=255
        q = r["qual"]
        with np.errstate(invalid="ignore"):  # (an infinite QUAL is 255 on either side)
            near = np.abs(q - np.round(q)) <= 1e-6
        assert not np.any(near & (np.round(q) >= 1) & (np.round(q) <= 255)), (name, q[near])
        assert np.all(r["margin"] > 1e-9), (name, r["margin"].min())  # nor a different flag
        base = 0
        for w, (start, ref, contig, samples) in enumerate(windows):
            n = len(ref)
            sl = slice(base, base + n)
            base += n
            if r["window_status"][w] != 0:
                seen["status %d" % r["window_status"][w]] += 1
                continue
            seen["empty window"] += n == 0
            seen["sample without reads"] += n > 0 and any(not s for s in samples) and any(s for s in samples)
            pos = start + np.arange(n)
            mean32 = r["soft_clip_mean"][sl].astype(np.float32)
            k = np.minimum(mean32, np.float32(reach)).astype(np.int64)
            clipped = mean32 >= np.float32(6.0)
            seen["mult > 1"] += int(np.sum(r["mult"][sl] > 1))
            seen["soft clips cut at position 0"] += int(np.sum(clipped & (pos - k < 0)))
            seen["soft clips cut at the contig length"] += int(np.sum(clipped & (pos + k > contig)))
            active = r["is_active_prob"][sl] > 0
            seen["band cut at position 0"] += int(np.sum(active & (pos - F < 0)))
            seen["band cut at the contig length"] += int(np.sum(active & (pos + F > contig)))
            seen["band reaches the contig length itself"] += int(np.sum(active & (pos + F >= contig) & (pos <= contig)))
            seen["called"] += int(np.sum(r["af_flags"][sl] & 1))
            seen["not called"] += int(np.sum(1 - (r["af_flags"][sl] & 1)))
            seen["profile boundary inside a window"] += bool(o["profile_size"] and o["profile_size"] < n)
            seen["window starts below F"] += 0 < start < F
            seen["last position is the contig's last base"] += n > 0 and start + n == contig
    for what in ("ins_entry", "ins_before_bound_start", "deletion_with_lagging_cig_index", "lagging_cig_index_changes_the_answer",
                 "ins_past_bound_end", "del_past_bound_end", "match_past_bound_end", "else_if_arm", "break_on_past_query_pos",
                 "uncounted_base", "soft_clips_added", "two_slots_of_one_read_at_one_position", "read_crosses_window_start",
                 "read_crosses_window_end"):
        assert total[what] > 0, what
    for what in ("status -1", "status -2", "empty window", "sample without reads", "mult > 1", "soft clips cut at position 0",
                 "soft clips cut at the contig length", "band cut at position 0", "band cut at the contig length",
                 "band reaches the contig length itself", "called", "not called", "profile boundary inside a window",
                 "window starts below F", "last position is the contig's last base"):
        assert seen[what] > 0, what
    # the uncounted mismatch beside a clip adds no soft clips, the counted one does
    assert K.restated("uncounted mismatch beside a clip")[0]["soft_clip_count"].sum() == 0
    assert K.restated("counted mismatch beside a clip")[0]["soft_clip_count"].sum() > 0
    # the two lagging cases flip the deletion's answer in either direction
    assert K.restated("lagging cig_index hides the soft clip")[0]["soft_clip_count"].sum() == 0
    assert K.restated("no lag: the same deletion inside the window")[0]["soft_clip_count"].sum() == 3
    assert K.restated("lagging cig_index finds a soft clip")[0]["soft_clip_count"].sum() == 3
    # an insertion's entry is decided by its first base against the reference base at its position
    assert K.restated("insertion whose first base matches")[0]["non_ref_depth"][20, 0] == 1
    assert K.restated("insertion whose first base differs")[0]["non_ref_depth"][20, 0] == 2
