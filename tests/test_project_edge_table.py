"""The inputs tests/test_project_edges_hip.py feeds phmm_project_to_reference, held against the sources and the oracle alone: the
constants the builders of tests/project_edge_cases.py assume are the ones in lorikeet_amd/csrc (a moved threshold fails here
until the batches sit at the new one), every input goes through the oracle, and the conditions that keep a device test from
passing on panics alone hold.  No GPU."""
import os
import re

import numpy as np
import pytest

import project_edge_cases as cases
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lorikeet_amd", "csrc")
LEGAL = "MIDS=X"     # the operators CigarPairTransform has rows for


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _function(text, name):
    m = re.search(r"\nhipError_t %s\(.*?\n\}\n" % re.escape(name), text, re.S)
    assert m, name
    return m.group(0)


def test_the_boundaries_are_the_sources():
    host, kernels, device, fused = _source("phmm_cigar.cpp"), _source("phmm_cigar_kernels.hip"), _source("phmm_cigar_device.hpp"), _source("phmm_sw.cpp")
    assert "const uint32_t capacity = 4 * (max_sw + max_hc + 2) + 8;" in host and cases.capacity(3, 4) == 4 * 9 + 8
    assert "const size_t ws_bytes = (size_t)n_reads * 4 * capacity * 4;" in host          # four builders of `capacity` words per read
    for name, count in (("launch_project", "n"), ("launch_pick", "p.n_reads")):
        body = _function(kernels, name)
        assert "const size_t lds_per_lane = 4ull * p.capacity * 4;" in body, name
        m = re.search(r"const bool in_lds = %s <= (\d+) && (\d+) \* lds_per_lane <= (\d+) \* 1024;" % re.escape(count), body)
        assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3)) * 1024) == (cases.LDS_MAX_READS, cases.LDS_BLOCK, cases.LDS_BYTES), name
        m = re.search(r"per_block = in_lds \? (\d+) : (\d+),", body)
        assert m and (int(m.group(1)), int(m.group(2))) == (cases.LDS_BLOCK, cases.HBM_BLOCK), name
        assert "in_lds ? %d * lds_per_lane : 0" % cases.LDS_BLOCK in body, name
    assert len(re.findall(r"__launch_bounds__\(%d\) void phmm_(?:project_kernel|pick_reads)\(" % cases.HBM_BLOCK, kernels)) == 2
    # 28 elements are the last launch in LDS, with exactly 64 KB -- the most a launch gets without a function attribute
    assert cases.LAST_LDS_N == 28 and cases.lds_bytes(28) == 65536 and cases.lds_bytes(29) > cases.LDS_BYTES
    assert {n for _, n in cases.COUNT_CASES} == {28, 29}
    # the fused call: the library's own alignment slots take max_sw's place
    assert re.search(r"uint32_t sw_capacity = %d;\s*// CIGAR elements reserved per alignment on the device" % cases.FUSED_SW_SLOTS, fused)
    assert "pj_capacity = 4 * (PJ->sw_capacity + PJ->max_hap_cigar + 2) + 8;" in fused
    # the short cut and the pad
    assert "(uint64_t)(uint32_t)sw_offset + read_len <= (uint64_t)len_of(hce) + %du;" % cases.PLAIN_PAD in device
    assert "CHECK(B.add(elem(OP_M, %d)));" % cases.PLAIN_PAD in device
    assert cases.PLAIN_DELTAS == (cases.PLAIN_PAD - 1, cases.PLAIN_PAD, cases.PLAIN_PAD + 1)


def _checked(inputs):
    """Every read through the oracle: a status the oracle has, and never its own capacity error."""
    expected = cases.oracle_all(inputs)
    assert len(expected) == inputs[0].n_reads
    for r, (st, pos, cig) in enumerate(expected):
        assert st in (0, 1, -1, -2, -3, -4, -5), cases.describe(inputs, r)
        assert st == 0 or (pos == 0 and cig == "")
    return expected


def _deterministic(build, *key):
    build.cache_clear()
    first = build(*key)
    build.cache_clear()
    second = build(*key)
    a, b = (first[0], second[0]) if isinstance(first[0], tuple) else (first, second)
    assert all(np.array_equal(getattr(a[0], f), getattr(b[0], f)) for f in a[0].FIELDS) and np.array_equal(a[1], b[1])
    assert all((x is None) == (y is None) and (x is None or (np.array_equal(x.elements, y.elements) and x.alignment_offset == y.alignment_offset))
               for x, y in zip(a[2], b[2]))
    assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3])) and a[4:7] == b[4:7] and all(np.array_equal(x, y) for x, y in zip(a[7], b[7]))
    return second


@pytest.mark.parametrize("flank,letters", cases.TABLE_CASES)
def test_operator_pair_table(flank, letters):
    inputs, where = _deterministic(cases.table, flank, letters)
    expected = _checked(inputs)
    assert sorted(where) == sorted((a, c) for a in cases.OPS for c in cases.OPS)
    aligned, hap_cigars, b, best = inputs[2], inputs[3], inputs[0], inputs[1]
    reg = cases.read_region(inputs)
    statuses = {}
    for (a, c), reads in where.items():
        # the issue's rows: `4M 3a 4M` at offsets 0 ... 8 against `6M 5c 200M`
        first = reads[:9]
        assert [aligned[r].alignment_offset for r in first] == list(range(9))
        for r in first:
            hp = int(b.region_hap_off[reg[r]]) + int(best[r])
            assert oracle.cigar_to_string(aligned[r].elements) == "4%s3%s4%s" % (flank, a, flank)
            assert oracle.cigar_to_string(hap_cigars[hp]) == "6%s5%s200%s" % (flank, c, flank)
            assert int(b.read_off[r + 1] - b.read_off[r]) == cases.read_len("4%s3%s4%s" % (flank, a, flank))
        statuses[a, c] = [expected[r][0] for r in reads]
        if a in LEGAL and c in LEGAL:
            # not all panics.  (An S between two aligned blocks is the builder's order error for every offset, on either
            # side: those pairs realign on the rows that carry the S at an end.)
            assert 0 in statuses[a, c], (a, c, statuses[a, c])
            if a != "S" and c != "S":
                assert 0 in statuses[a, c][:9], (a, c, statuses[a, c])
            else:
                assert set(statuses[a, c][:9]) == {-1}, (a, c, statuses[a, c])
    assert inputs[0].n_reads >= 81 * 9 and len(set(bytes(inputs[0].hap_bases))) == letters
    assert any(st == -5 for (a, c), sts in statuses.items() if a in "NHP" or c in "NHP" for st in sts)   # the pairs without a transform


@pytest.mark.parametrize("letters", (4, 2))
def test_builder_rules(letters):
    inputs = _deterministic(cases.rules, letters)
    expected = _checked(inputs)
    want = ["3D5M", "2I3D5M", "2S3D5M", "2H2S3D5M", "5M3D", "5M3D2I", "5M3D2S", "5M3D2I2S", "5M2I3D4M", "5M3D2I3D4M", "5M0D4M", "0M5M",
            "5M2S3M", "5M2H2S", "5S", "3D", "2I", "3D2I", "5M3N4M", "5M2P4M"]
    assert cases.RULE_ALIGNMENTS[:len(want)] == want
    seen = {}
    for r, a in enumerate(inputs[2]):
        aln = oracle.cigar_to_string(a.elements)
        assert int(inputs[0].read_off[r + 1] - inputs[0].read_off[r]) == cases.read_len(aln)
        seen.setdefault(aln, set()).add(expected[r][0])
    assert set(seen) == set(cases.RULE_ALIGNMENTS) and inputs[0].n_reads == len(cases.RULE_ALIGNMENTS) * 3 * 2 * 5
    assert {oracle.cigar_to_string(c) for c in inputs[3]} == {"120M", "20M2D98M", "20M2I100M"}
    assert {re.sub(r"\d+M", "nM", oracle.cigar_to_string(c)) for c in inputs[7]} == {"nM", "3H2SnM1S", "2SnM4H", "5S", "2H"}
    # the rules: the order error, "completely soft clipped", "last element cannot be None"; a stripped deletion realigns
    assert seen["5M2S3M"] == {-1} and seen["5M2H2S"] == {-1} and seen["5S"] == {-2} and seen["3D"] == {-3} and seen["0D5M0I"] <= {0, -5}
    for aln in ("3D5M", "2S3D5M", "5M3D", "5M3D2I", "5M3D2S", "5M3D2I2S", "5M2I3D4M", "5M3D2I3D4M", "5M0D4M", "0M5M", "2I", "3D2I"):
        assert 0 in seen[aln], (aln, seen[aln])
    assert seen["5M3N4M"] == {-5} and seen["5M2P4M"] == {-5}


def _indels(text):
    return sum(o in "ID" for _, o in cases.elements(text))


def _aligned_before_first_indel(text):
    n = 0
    for k, o in cases.elements(text):
        if o in "ID":
            return n
        n += k if o in "M=X" else 0
    return None


@pytest.mark.parametrize("u", sorted(cases.UNITS))
def test_repeats(u):
    inputs = _deterministic(cases.repeats, u)
    expected = _checked(inputs)
    b, best, aligned, hap_cigars, hap_starts, ref_hap, ref_start, orig = inputs
    reg = cases.read_region(inputs)
    moved = merged = shifted = past_end = 0
    for r, (st, pos, cig) in enumerate(expected):
        g = int(reg[r])
        hp = int(b.region_hap_off[g]) + int(best[r])
        aln = oracle.cigar_to_string(aligned[r].elements)
        assert int(b.read_off[r + 1] - b.read_off[r]) == cases.read_len(aln)
        past_end += st == -5
        if st != 0:
            continue
        start = oracle.read_start_on_reference_haplotype(oracle.consolidated_padded_cigar(hap_cigars[hp], 1000), aligned[r].alignment_offset)
        moved += pos != ref_start[g] + hap_starts[hp] + start
        merged += _indels(cig) < _indels(aln)
        if len(hap_cigars[hp]) == 1 and _indels(aln) == 1 and _indels(cig) == 1 and aln[0] != "3":
            shifted += _aligned_before_first_indel(cig) <= _aligned_before_first_indel(aln) - 1
    assert moved >= 20 and merged >= 20 and shifted >= 20 and past_end >= 20, (moved, merged, shifted, past_end)
    offsets = {a.alignment_offset for a in aligned}
    assert 0 in offsets and max(offsets) > 0 and {0, 3, 7} <= set(hap_starts)
    assert {len(c) for c in hap_cigars} == {1, 3}


def test_plain_boundary():
    inputs, rows = _deterministic(cases.plain)
    expected = _checked(inputs)
    b, aligned, hap_cigars = inputs[0], inputs[2], inputs[3]
    reg = cases.read_region(inputs)
    sides = {}
    same = {}
    for r, kind, delta, longer in rows:
        hp = int(b.region_hap_off[reg[r]]) + int(inputs[1][r])
        n_aln = cases.read_len(oracle.cigar_to_string(aligned[r].elements))
        assert aligned[r].alignment_offset + n_aln - (int(hap_cigars[hp][0]) >> 4) == delta and len(hap_cigars[hp]) == 1
        assert int(b.read_off[r + 1] - b.read_off[r]) == n_aln + longer
        assert (len(aligned[r].elements) == 1) == (kind == "plain")
        st = expected[r][0]
        sides.setdefault(delta <= cases.PLAIN_PAD, set()).add(st == 0)
        if kind == "plain" and longer == 0:
            sides.setdefault(("short cut", delta), set()).add(st)
        same.setdefault((aligned[r].alignment_offset, n_aln, hp, longer), set()).add(st)
    assert sides[True] == sides[False] == {True, False}                    # realigned and refused reads on both sides of the line
    assert sides["short cut", 999] == sides["short cut", 1000] == {0} and sides["short cut", 1001] == {-5}
    assert all(len(v) == 1 for v in same.values()) and len(same) * 3 == len(rows)   # the three spellings of a read: one status
    lens = np.diff(b.read_off.astype(np.int64))
    assert (lens == 0).sum() >= 9 and {a.alignment_offset for a in aligned} >= {0, -1, -2}
    empty = [expected[r][0] for r in range(b.n_reads) if lens[r] == 0]
    assert set(empty) >= {1, -3, -5}


@pytest.mark.parametrize("cls", range(len(cases.RANDOM_CLASSES)))
def test_random_alignments(cls):
    inputs = _deterministic(cases.random_alignments, cls)
    expected = _checked(inputs)
    aln_ops, hap_ops = cases.RANDOM_CLASSES[cls]
    b, best, aligned, hap_cigars = inputs[:4]
    assert b.n_reads == cases.RANDOM_READS
    assert {cases.OPS[int(e) & 15] for a in aligned for e in a.elements} == set(aln_ops)
    assert {cases.OPS[int(e) & 15] for c in hap_cigars for e in c} == set(hap_ops)
    assert {len(c) for c in hap_cigars} == {1, 2, 3, 4, 5}
    n_aln = [len(a.elements) for a in aligned]
    assert min(n_aln) == 1 and max(n_aln) == (8 if aln_ops == cases.OPS else 6)     # (all nine: a clip on either side on top)
    zero = np.mean([(int(e) >> 4) == 0 for a in aligned for e in a.elements])
    assert 0.03 < zero < 0.07
    off_by = np.mean([int(b.read_off[r + 1] - b.read_off[r]) != cases.read_len(oracle.cigar_to_string(a.elements)) for r, a in enumerate(aligned)])
    assert 0.08 < off_by < 0.18       # 15 % drawn, a fifth of them by 0
    assert {a.alignment_offset for a in aligned} >= set(range(30)) | {-1, -2, 2000}
    assert cases.histogram(expected).get(0, 0) >= 100


def test_random_alignments_reach_every_status():
    total = {}
    for cls in range(len(cases.RANDOM_CLASSES)):
        for st, n in cases.histogram(cases.oracle_all(cases.random_alignments(cls))).items():
            total[st] = total.get(st, 0) + n
    assert all(total.get(st, 0) >= 50 for st in (1, -1, -2, -3, -5)), total
    assert -6 not in total


@pytest.mark.parametrize("n_total", (27, 28, 29))
def test_workspace_boundary(n_total):
    inputs, long_read, pad = _deterministic(cases.workspace, n_total)
    expected = _checked(inputs)
    base = cases.random_alignments(*cases.WORKSPACE_BASE)
    max_sw, max_hc = cases.host_max(inputs)
    assert max_hc == max(len(c) for c in base[3]) and pad == n_total - max_hc
    assert max_sw + max_hc == n_total and len(inputs[2][long_read].elements) == max_sw == pad
    assert sorted(len(a.elements) for a in inputs[2])[-2] <= 8                        # all other reads stay short
    assert expected[long_read][0] == 0 and long_read == base[0].n_reads == inputs[0].n_reads - 1
    assert re.fullmatch(r"(2S)?(3M1[ID])*3M", oracle.cigar_to_string(inputs[2][long_read].elements))
    # the reads common to the three runs are the random batch itself
    assert expected[:long_read] == cases.oracle_all(base)
    assert (cases.lds_bytes(n_total) <= cases.LDS_BYTES) == (n_total <= 28)


@pytest.mark.parametrize("n_reads,n_total", cases.COUNT_CASES)
def test_read_counts(n_reads, n_total):
    inputs = cases.count(n_reads, n_total)
    expected = _checked(inputs)
    assert inputs[0].n_reads == n_reads and sum(cases.host_max(inputs)) == n_total and cases.host_max(inputs)[1] == cases.COUNT_MAX_HC
    assert expected[0][0] == 0 and len(inputs[2][0].elements) == n_total - cases.COUNT_MAX_HC
    assert np.diff(inputs[0].read_off.astype(np.int64))[1:].max(initial=0) <= 20     # short reads at the large counts
    assert cases.histogram(expected).get(0, 0) > n_reads // 2
    if n_reads > 1:   # a prefix of the longest batch, read by read
        longest = cases.count(4097, n_total)
        assert expected == cases.oracle_all(longest)[:n_reads]
    # the partial last block: in both block sizes for the counts that are no multiple of 64
    assert {n % cases.LDS_BLOCK for n, _ in cases.COUNT_CASES} >= {0, 1, 31} and {n % cases.HBM_BLOCK for n, _ in cases.COUNT_CASES} >= {0, 1, 63}
