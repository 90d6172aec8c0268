"""CPU checks around phmm_finalize_reads: the restatement (tests/finalize_restatement.py) held to the reference's own tests in
tests/read_clipper_unit_tests.rs, property for property, over the CIGAR family those tests run on
(tests/golden/read_clipper_cases.json, made by tests/golden/make_read_clipper_cases.py), to test_finalize_region's two mates,
and a census of the sets tests/test_finalize_hip.py runs on the GPU, so that none of them is vacuous.  The reference has no
asserting test of the pair step (test_finalize_region only runs it): that step is pinned by reading alone.  The module imports
lorikeet_amd.finalize at the top: without the call every test here fails."""
import os
import re
from collections import Counter

import pytest

import finalize_cases as K
import finalize_restatement as R
from conftest import ROOT
from lorikeet_amd import _lib, finalize  # noqa: F401

G = K.GOLDEN
CIGARS = G["cigars"]


def make_read(cigar, quals=None, pos=None):
    """ReadClipperTestUtils::make_read_from_cigar: (Read, qualities)"""
    rd = K.read(cigar, pos=pos, quals=quals)
    return R.Read(rd["pos"], 0, 60, -1, 0, rd["cigar"], len(rd["bases"])), rd["quals"]


def soft_end(r):
    end = r.get_end()
    found = False
    for op, n in reversed(r.cigar):
        if op == R.S:
            end += n
        elif op != R.H:
            found = True
            break
    return end if found else r.get_end()


def unclipped_limits(r):
    start, end = r.get_start(), r.get_end()
    for op, n in r.cigar:
        if not R.is_clipping(op):
            break
        start -= n
    for op, n in reversed(r.cigar):
        if not R.is_clipping(op):
            break
        end += n
    return start, end


def assert_consistent(r):
    """assert_ref_alignment_consistent and assert_read_length_consistent"""
    assert r.reference_length() == (0 if r.is_unmapped else r.get_end() - r.get_start() + (1 if r.reference_length() else 0))
    assert r.seq_len_from_cigar() == r.length, R.cigar_string(r.cigar)


def test_the_golden_file_is_what_its_maker_describes():
    assert len(CIGARS) == len(set(CIGARS)) == 217 and CIGARS[-1] == "2M3I5M"
    assert G["bases"] == "ACTG" and G["quals"] == [2, 15, 25, 30] and G["position"] == 10000 and G["maximum_cigar_elements"] == 6
    assert all(1 <= len(K.read(c)["bases"]) <= 12 for c in CIGARS)
    assert all(len(R.parse_cigar(c)) <= 6 for c in CIGARS)
    assert len(G["before_contig"]) == 6 and len(G["finalize_region"]["sam"]) == 2


def test_the_export_is_in_the_library_the_binding_and_the_rust_declarations():
    lib = _lib.load()
    ffi = open(os.path.join(ROOT, "integration", "hip_ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "phmm.h")).read()
    n = "phmm_finalize_reads"
    assert getattr(lib, n) is not None
    assert re.search(r"pub fn %s\s*\(" % n, ffi) and re.search(r"\bint %s\(" % n, header)
    args = next(a for name, _, a in _lib.SYMBOLS if name == n)
    decl = re.search(r"pub fn phmm_finalize_reads\s*\(([^)]*)\)", ffi, re.S).group(1)
    assert len(args) == len([x for x in decl.split(",") if x.strip()]) == 30
    for name in ("SOFT_CLIPS", "LOW_QUAL_ENDS", "ADAPTOR", "REGION", "PAIRS", "ALL", "STATUS_CIGAR", "STATUS_CLIP_RANGE", "STATUS_ARITHMETIC",
                 "STATUS_PAIR", "STATUS_WORKSPACE"):
        value = int(re.search(r"#define PHMM_FIN_%s \(?(-?\d+)u?\)?" % name, header).group(1))
        assert getattr(_lib, "PHMM_FIN_" + name) == value, name
        assert re.search(r"pub const PHMM_FIN_%s: \w+ = %d;" % (name, value), ffi), name
    assert (R.FIN_SOFT_CLIPS, R.FIN_LOW_QUAL_ENDS, R.FIN_ADAPTOR, R.FIN_REGION, R.FIN_PAIRS, R.FIN_ALL) == (1, 2, 4, 8, 16, 31)
    import tools.source_hash as SH
    assert "phmm_finalize_kernels.hip" in SH.KERNEL_SOURCES["finalize"]
    assert "finalize=%s" % SH.source_hash("finalize") in lib.phmm_build_info().decode()


def test_hard_clip_both_ends_by_reference():
    for c in CIGARS:
        read, _ = make_read(c)
        aln_start, aln_end = read.get_start(), read.get_end()
        read_length = aln_start - aln_end
        for i in range(int(read_length / 2) + 1, 1):     # (read_length / 2) + 1..=0 with Rust's division towards zero
            clipped, _ = make_read(c)
            R.hard_clip_both_ends_by_reference_coordinates(clipped, aln_start + i, aln_end - i)
            assert clipped.get_start() >= aln_start + i, c
            assert clipped.get_end() <= aln_end - i, c


def test_hard_clip_by_reference_coordinates():
    for c in CIGARS:
        read, _ = make_read(c)
        start, stop = max(read.get_soft_start_i64(), 0), soft_end(read)
        for i in range(start, stop + 1):
            left, _ = make_read(c)
            R.clip_by_reference_coordinates(left, None, i)
            if not left.is_empty():
                assert left.get_start() >= min(read.get_end(), i), (c, i)
                assert_consistent(left)
            right, _ = make_read(c)
            R.clip_by_reference_coordinates(right, i, None)
            if not right.is_empty() and right.get_start() <= right.get_end():
                assert right.get_end() <= max(read.get_start(), i), (c, i)
                assert_consistent(right)


def test_hard_clip_by_reference_coordinates_left_and_right_tail():
    for c in CIGARS:
        read, _ = make_read(c)
        aln_start, aln_end = read.get_start(), read.get_end()
        for i in range(aln_start, aln_end + 1):
            if read.get_soft_start() == aln_start:
                left, _ = make_read(c)
                R.clip_by_reference_coordinates(left, None, i)
                if not left.is_empty():
                    assert left.get_start() >= i, (c, i)
                    assert_consistent(left)
            if soft_end(read) == aln_start:
                right, _ = make_read(c)
                R.clip_by_reference_coordinates(right, i, None)
                if not right.is_empty() and right.get_start() <= right.get_end():
                    assert right.get_end() <= i, (c, i)
                    assert_consistent(right)


def test_hard_clip_low_qual_ends():
    low, high = 2, 30
    for c in CIGARS:
        n = len(K.read(c)["bases"])
        for k in range(n):
            patterns = [[low] * k + [high] * (n - k), [high] * (n - k) + [low] * k]
            if k <= n // 2:
                patterns.append([low] * k + [high] * (n - 2 * k) + [low] * k)
            for quals in patterns:
                read, _ = make_read(c, quals)
                R.hard_clip_low_qual_ends(read, quals, low)
                if not read.is_empty():   # assert_no_low_qual_bases
                    assert all(q > low for q in quals[read.first:read.first + read.length]), (c, quals)


def test_hard_clip_soft_clipped_bases():
    for c in CIGARS:
        read, _ = make_read(c)
        clipped, _ = make_read(c)
        R.hard_clip_soft_clipped_bases(clipped)
        if clipped.is_empty():
            continue
        if any(not R.is_clipping(op) for op, _ in read.cigar):   # assert_unclipped_limits
            assert unclipped_limits(read) == unclipped_limits(clipped), c
        before, after = Counter(), Counter()
        for op, n in read.cigar:
            before[op] += n
        for op, n in clipped.cigar:
            after[op] += n
        for op in before:                                          # assert_hard_clipping_soft_clips
            if R.is_clipping(op):
                assert before[R.H] + before[R.S] == after[R.H] and after[R.S] == 0, c
            else:
                assert before[op] == after[op], c


def leading(cigar, wanted):
    for op, n in cigar:
        if op == wanted:
            return n
        if op != R.H:
            return 0
    return 0


def test_revert_soft_clipped_bases():
    for c in CIGARS:
        read, _ = make_read(c)
        lead, tail = leading(read.cigar, R.S), leading(read.cigar[::-1], R.S)
        unclipped, _ = make_read(c)
        R.revert_soft_clipped_bases(unclipped)
        if any(not R.is_clipping(op) for op, _ in read.cigar):
            assert unclipped_limits(read) == unclipped_limits(unclipped), c
        if lead > 0 or tail > 0:
            assert unclipped.get_start() == read.get_start() - lead, c
            assert unclipped.get_end() == read.get_end() + tail, c
        else:
            assert unclipped.cigar == read.cigar


def test_revert_entirely_soft_clipped_reads():
    read, _ = make_read(G["entirely_soft_clipped"])
    clipped, _ = make_read(G["entirely_soft_clipped"])
    R.revert_soft_clipped_bases(clipped)
    assert clipped.get_start() == read.get_soft_start()


@pytest.mark.parametrize("case", G["before_contig"], ids=lambda c: "%d_%d" % (c["soft_start"], c["alignment_start"]))
def test_revert_soft_clips_before_contig(case):
    read, _ = make_read(case["cigar"], pos=case["alignment_start"])
    assert read.get_soft_start_i64() == case["soft_start"] and read.get_start() == case["alignment_start"]
    R.revert_soft_clipped_bases(read)
    assert read.get_soft_start_i64() == case["expected_start"] and read.get_start() == case["expected_start"]
    assert R.cigar_string(read.cigar) == case["expected_cigar"]


def test_finalize_region_changes_the_qualities_of_both_mates_in_their_overlap():
    """test_finalize_region: mates that overlap one another without agreement have modified base qualities afterwards"""
    fr = G["finalize_region"]
    reads = []
    for line in fr["sam"]:
        f = line.split("\t")
        reads.append(dict(pos=int(f[3]) - 1, flags=int(f[1]), mapq=int(f[4]), cigar=f[5], mpos=int(f[7]) - 1, isize=int(f[8]), bases=f[9].encode(),
                          quals=[ord(ch) - 33 for ch in f[10]], mate=1 - len(reads)))
    span = (max(fr["span"][0] - fr["extension"], 0), min(fr["span"][1] + fr["extension"], fr["contig_length"]))
    a, b = R.finalize_reads([dict(span=span, reads=reads)], steps=R.FIN_ALL, min_tail_quality=fr["min_bq"])
    assert a["read_status"] == b["read_status"] == 0 and a["keep"] == b["keep"] == 1
    changed = [[i for i, (x, y) in enumerate(zip(r["out_quals"], rd["quals"])) if x != y] for r, rd in zip((a, b), reads)]
    assert changed[0] and changed[1]
    # the changes lie in the overlap: the last bases of the first read's window, the first of the second's
    assert min(changed[0]) >= a["clip_first"] + a["clip_len"] - len(range(b["new_pos"], a["new_pos"] + 200)) and max(changed[0]) < a["clip_first"] + a["clip_len"]
    assert min(changed[1]) >= b["clip_first"] and len(changed[0]) == len(changed[1])
    assert all(q <= 20 for r in (a, b) for i, q in enumerate(r["out_quals"]) if i in changed[(a, b).index(r)])


# ---- what the GPU sets exercise ---------------------------------------------------------------------------------------------

def test_census_of_the_gpu_sets():
    statuses, keeps, steps = Counter(), Counter(), 0
    for name, groups, options in K.sets():
        res = K.restated(name)
        assert len(res) == sum(len(g["reads"]) for g in groups), name
        statuses.update(r["read_status"] for r in res)
        keeps.update(r["keep"] for r in res)
        steps |= options["steps"]
        if name.startswith("random"):
            assert len(res) == 2000 and len(groups) == 40
            assert sum(r["read_status"] < 0 for r in res) <= 0.02 * len(res), name
            reads = [rd for g in groups for rd in g["reads"]]
            assert sum(r["out_quals"] != list(rd["quals"]) for r, rd in zip(res, reads)) > 200   # pairs that overlap
            assert sum(r["clip_first"] > 0 for r in res) > 200 and sum(0 < r["clip_len"] < len(rd["bases"]) for r, rd in zip(res, reads)) > 400
            assert sum(r["out_unmapped"] for r in res) > 20
    assert steps == R.FIN_ALL
    for status in (0, R.STATUS_CIGAR, R.STATUS_CLIP_RANGE, R.STATUS_ARITHMETIC, R.STATUS_PAIR):
        assert statuses[status] > 0, status
    assert keeps[0] > 0 and keeps[1] > 0
    # each single step alone is one of the sets, and every step changes something there
    alone = {options["steps"] for _, _, options in K.sets()}
    assert {R.FIN_SOFT_CLIPS, R.FIN_LOW_QUAL_ENDS, R.FIN_ADAPTOR, R.FIN_REGION, R.FIN_PAIRS, R.FIN_ALL} <= alone
    for name in ("soft clips hard-clipped", "soft clips by fragment", "low-quality tails", "adaptor", "region", "all steps", "tail scan"):
        _, groups, _ = K.case(name)
        reads = [rd for g in groups for rd in g["reads"]]
        assert sum(r["clip_len"] != len(rd["bases"]) or r["out_cigar"] != R.parse_cigar(rd["cigar"]) for r, rd in zip(K.restated(name), reads)) > 50, name


def test_census_of_the_edge_sets():
    res, (_, groups, _) = K.restated("edges"), K.case("edges")
    reads = [rd for g in groups for rd in g["reads"]]
    assert {1, 2, 200} <= {len(R.parse_cigar(rd["cigar"])) for rd in reads if isinstance(rd["cigar"], str)}
    assert any(r["new_pos"] == 0 and r["out_cigar"] and r["out_cigar"][0] == (R.H, 11) for r in res)   # reverted below the contig's start
    assert any(r["out_cigar"] == [(R.M, 0)] for r in res)                                               # flagged unmapped
    assert any(r["out_unmapped"] for r in res) and any(len(rd["bases"]) == 0 for rd in reads)
    kept_soft = K.restated("region")   # (the soft-clip step leaves none: the sets without it hold them)
    assert any(r["lead_soft"] for r in kept_soft) and any(r["trail_soft"] for r in kept_soft)
    scan = K.restated("tail scan")
    assert {r["clip_len"] for r in scan} >= {0, 1, 15, 16, 17, 63, 64, 65, 300}
    pairs, (_, pgroups, _) = K.restated("pairs"), K.case("pairs")
    preads = [rd for g in pgroups for rd in g["reads"]]
    touched = [sum(x != y for x, y in zip(r["out_quals"], rd["quals"])) for r, rd in zip(pairs, preads)]
    assert {1, 63, 64, 65, 100} <= set(touched)
    assert any(0 in r["out_quals"] for r in pairs) and any(20 in r["out_quals"] for r in pairs)
    panics = K.restated("pair panics")
    assert [r["read_status"] for r in panics] == [R.STATUS_ARITHMETIC] * 2 + [0, 0] + [R.STATUS_PAIR] * 2 + [0]
    assert panics[2]["out_quals"] != K.case("pair panics")[1][1]["reads"][0]["quals"]
