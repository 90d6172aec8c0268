"""CPU: holds tests/region_trim_restatement.py to the literals of the reference's own tests (tests/golden/region_trim_cases.json:
Haplotype::trim, trim_cigar_by_reference, the shape of trim_to's test), to one hand-derived expectation per quirk that the
reference has no test of (AssemblyRegionTrimmer, get_variation_events, the order of trim_down_haplotypes), runs
get_num_tandem_repeat_units itself over every small biallelic indel, and counts what the GPU case sets reach."""
import itertools
import json
import os
import re

import events_restatement as EV
import region_trim_cases as K
import region_trim_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "region_trim_cases.json")))
P = EV.parse_cigar


def cs(cigar):
    return "".join("%d%s" % (n, EV.OPS[op]) for op, n in cigar)


# ---- the layers agree ---------------------------------------------------------------------------------------------------------------
def test_the_module_the_header_and_the_restatement_name_the_same_values():
    from lorikeet_amd import _lib, trim
    header = open(os.path.join(ROOT, "include", "phmm.h")).read()
    defines = {k: int(v) for k, v in re.findall(r"#define PHMM_TRIM_(\w+) \(?(-?\d+)u?\)?", header)}
    assert len(defines) == 14
    for name, value in defines.items():
        assert getattr(trim, name) == value, name
    for name in ("LOCATION", "LENGTH", "OPERATOR", "NOT_FOUND", "BUILDER", "REF_ELIMINATED", "REPEAT_SLICE"):
        assert getattr(R, name) == defines["STATUS_" + name]
    for name in ("DUPLICATE", "CUT_IN_DELETION", "EMPTY", "ALL_INSERTION", "NOT_TRIMMED"):
        assert getattr(R, name) == defines["FATE_" + name]
    assert (R.VARIATION_SPAN, R.VARIATION_SET) == (defines["VARIATION_SPAN"], defines["VARIATION_SET"])
    internal = open(os.path.join(ROOT, "lorikeet_amd", "csrc", "phmm_trim_internal.hpp")).read()
    for name, value in defines.items():
        key = name.replace("STATUS_", "")
        assert re.search(r"TRIM_%s = %d\b" % (key, value), internal), name
    assert any(s[0] == "phmm_trim_regions" and len(s[2]) == 41 for s in _lib.SYMBOLS)


def test_the_library_carries_the_trim_family_hash_and_the_layers_bind_the_export():
    from lorikeet_amd import _lib
    import lorikeet_amd
    import tools.source_hash as SH
    lib = _lib.load()
    assert "trim=%s" % SH.source_hash("trim") in lib.phmm_build_info().decode()
    assert lorikeet_amd.trim_regions is lorikeet_amd.trim.trim_regions
    backend = open(os.path.join(ROOT, "integration", "hip_backend.rs")).read()
    assert "pub fn trim_regions(" in backend and "phmm_trim_regions(" in backend


# ---- the reference's own tests --------------------------------------------------------------------------------------------------------
def test_trimming_every_sub_span_of_an_all_m_haplotype():
    c = GOLDEN["test_trimming"]
    loc, bases, hs = c["loc"], c["bases"].encode(), c["hap_start"]
    n = 0
    for trim_start in range(loc[0], loc[1]):
        for trim_stop in range(trim_start, loc[1] + 1):
            start, stop = trim_start - loc[0], trim_start - loc[0] + (trim_stop - trim_start) + 1
            got = R.haplotype_trim((bases, [(R.OP_M, len(bases))], hs, tuple(loc), False), (start + loc[0], stop + loc[0] - 1))
            assert got == (bases[start:stop], [(R.OP_M, stop - start)], hs + start)
            n += 1
    assert n == 65


def test_trimming_into_a_deletion_is_none():
    c = GOLDEN["test_trimming_none"]
    assert len(c["spans"]) == 3
    for span in c["spans"]:
        assert R.haplotype_trim((c["bases"].encode(), P(c["cigar"]), c["hap_start"], tuple(c["loc"]), False), tuple(span)) == R.CUT_IN_DELETION


def test_trimming_with_leading_and_trailing_insertions():
    c = GOLDEN["test_trimming_data_with_leading_and_trailing_insertions"]
    off = c["offset"]
    assert len(c["rows"]) == 5
    for bases, cigar, start, stop, want_cigar, want_bases in c["rows"]:
        ref_len = sum(n for op, n in P(cigar) if R.consumes_ref(op))
        got = R.haplotype_trim((bases.encode(), P(cigar), off, (off, off + ref_len - 1), False), (off + start, off + stop))
        assert (got[0].decode(), cs(got[1]), got[2]) == (want_bases, want_cigar, off + start)


def test_bad_trim_loc():
    import pytest
    c = GOLDEN["test_bad_trim_loc"]
    with pytest.raises(R.Panic) as e:
        R.haplotype_trim((c["bases"].encode(), [(R.OP_M, len(c["bases"]))], 0, tuple(c["loc"]), False), tuple(c["span"]))
    assert e.value.status == R.LOCATION


def expected_through_a_builder(text):
    """test_trim_cigar: a lone deletion is skipped, everything else goes through CigarBuilder::new(true)"""
    raw = P(text)
    if len(raw) == 1 and raw[0][0] == R.OP_D:
        return None
    b = R.CigarBuilder(True)
    for op, n in raw:
        assert b.add(op, n)
    return b.make()


def test_make_trim_cigar_data():
    c = GOLDEN["make_trim_cigar_data"]
    n = 0
    for op in c["ops"]:
        for my_length in range(*c["my_length"]):
            for start in range(0, my_length - 1):
                for end in range(start, my_length):
                    for pad_op in c["pad_ops"]:
                        for left in range(*c["pad"]):
                            for right in range(*c["pad"]):
                                text = ("%d%s" % (left, pad_op) if left else "") + "%d%s" % (my_length, op) + ("%d%s" % (right, pad_op) if right else "")
                                want = expected_through_a_builder("%d%s" % (end - start + 1, op))
                                if want is not None:
                                    assert R.trim_cigar_by_reference(P(text), start + left, end + left) == want, text
                                    n += 1
    for left in c["insertion_pads"]:
        for right in c["insertion_right_pads"]:
            if left + right > 0:
                for ins in c["insertion_sizes"]:
                    for start in range(0, left + 1):
                        for stop in range(left, left + right):
                            l, r = left - start, stop - left + 1
                            want = expected_through_a_builder(("%dM" % l if l else "") + "%dI" % ins + ("%dM" % r if r else ""))
                            assert R.trim_cigar_by_reference(P("%dM%dI%dM" % (left, ins, right)), start, stop) == want
                            n += 1
    for text, start, end, want in c["rows"]:
        want = expected_through_a_builder(want)
        if want is not None:
            assert R.trim_cigar_by_reference(P(text), start, end) == want, (text, start, end)
            n += 1
    assert n > 300 and len(c["rows"]) == 16


def test_trimming_data_shape_with_fixed_bases():
    """trimming_data: the reference haplotype and eleven haplotypes with one substitution each at base 0 .. 10 of the padded
    span, all M; trimmed to the middle of the padded span every one of them equals the reference there, and the reference wins"""
    c = GOLDEN["trimming_data"]
    a0, a1 = c["active"]
    p0, p1 = a0 - c["padding"], a1 + c["padding"]
    import random
    ref = K.rand_ref(random.Random(1), p1 - p0 + 1)
    haps = [K.make_hap(ref, p0, (), True)] + [K.make_hap(ref, p0, K.snps(ref, [i])) for i in range(c["haplotypes"][0], c["haplotypes"][1] + 1)]
    length = p1 - p0 + 1
    new_loc = (p0 + length // 2, p1 - length // 2)
    items, fates, dup_of = R.trim_down_haplotypes(new_loc, [(h[0], list(h[1]), h[2], h[3], h[4]) for h in haps])
    assert len(haps) == 12 and len(items) == 1 and items[0][1] == 0 and items[0][0][3] is True
    assert len(items[0][0][0]) == new_loc[1] - new_loc[0] + 1
    assert fates == [0] + [R.DUPLICATE] * 11 and dup_of == [R.NONE32] + [0] * 11


# ---- get_num_tandem_repeat_units: the STR arm has no input ----------------------------------------------------------------------------
def test_no_biallelic_indel_has_repeat_units():
    """every biallelic indel with up to 4 inserted or deleted bases over {A, C} on a few repeat contexts, the doc comment's
    TCCA -> T among them: get_num_tandem_repeat_units is None throughout, as written (Some needs `lengths` EMPTY, :74)"""
    contexts = [b"CCACCACCAGTCGA", b"AAAAAAAAAAAA", b"ACACACACACAC", b"CCCCAAAACCCC", b"AACAACAACAAC", b"", b"A", b"CA"]
    seqs = [bytes(s) for n in range(1, 5) for s in itertools.product(b"AC", repeat=n)]
    n = 0
    for pad in (b"T", b"A"):
        for seq in seqs:
            for context in contexts:
                for ref, alt in ((pad + seq, pad), (pad, pad + seq)):
                    assert R.get_num_tandem_repeat_units(True, ref, [alt], context) is None, (ref, alt, context)
                    n += 1
    assert R.get_num_tandem_repeat_units(True, b"TCCA", [b"T"], b"CCACCACCAGTCGA") is None
    assert n == 2 * 30 * 8 * 2
    # what the pieces do on the way: only homopolymers decompose, and those push two lengths
    assert R.find_repeated_substring(b"CC") == 1 and R.find_repeated_substring(b"CACA") == 0 and R.find_repeated_substring(b"C") == 0
    assert R.get_num_tandem_repeat_units_main(b"", b"AA", b"AAAC") == ([3, 5], b"A")
    assert R.get_num_tandem_repeat_units(True, b"T", [], b"AAA") == ([], b"")      # the only Some: no alternate allele
    assert R.get_num_tandem_repeat_units(False, b"T", [b"C"], b"AAA") is None


# ---- one hand-derived expectation per quirk -------------------------------------------------------------------------------------------
def test_the_two_overlap_tests_agree_on_well_formed_intervals():
    for a in itertools.combinations_with_replacement(range(6), 2):
        for b in itertools.combinations_with_replacement(range(6), 2):
            assert R.overlaps(a, b) == R.coord_overlaps(a[0], a[1], b[0], b[1]) == (a[0] <= b[1] and b[0] <= a[1])


REF = b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT"    # 40 bases from 1000


def one(haps, active=(1010, 1029), padded=(1000, 1039), padding=(2, 5, 9, 0), ref=REF):
    return R.trim_region((ref, 1000, active, padded, [K.make_hap(ref, 1000, e, r) for e, r in haps]), 0, padding)


def test_spans_by_hand():
    r = one([((), True), ([("S", 15, ord("A"))], False)])                       # one SNP at 1015, padding 2
    assert (r["variant"], r["padded"], r["variation"]) == ((1015, 1015), (1013, 1017), 3)
    assert (r["new_active"], r["new_padded"]) == ((1015, 1015), (1013, 1017))
    r = one([((), True), ([("S", 15, ord("A")), ("I", 20, b"GG")], False)])      # + an insertion at 1019, padding 5
    assert (r["variant"], r["padded"]) == ((1015, 1019), (1013, 1024))
    r = one([((), True), ([("D", 8, 5)], False)])                                # a deletion 1007 .. 1012 that only ENDS inside
    assert (r["variant"], r["padded"]) == ((1010, 1012), (1002, 1017))           # the span is cut to the active span, the padding is not
    r = one([((), True), ([("S", 5, ord("T"))], False)])                         # an event in the padding only
    assert (r["variation"], r["out"], r["fates"]) == (0, [], [R.NOT_TRIMMED] * 2)
    r = one([((), True), ([("S", 11, ord("A")), ("D", 26, 2)], False)], padded=(1010, 1030))   # 1009 and 1032: cut on both sides
    assert (r["variant"], r["padded"]) == ((1011, 1027), (1010, 1030))
    r = one([((), True), ([("S", 12, ord("T")), ("I", 13, b"AA")], False)])      # a SNP joined with an insertion keeps the SNP's padding
    assert (r["variant"], r["padded"]) == ((1012, 1012), (1010, 1014))


def test_a_start_smaller_than_its_padding_saturates():
    r = R.trim_region((REF, 0, (2, 30), (0, 39), [K.make_hap(REF, 0, (), True), K.make_hap(REF, 0, [("S", 3, ord("A"))])]), 0, (20, 75, 75, 0))
    assert (r["variant"], r["padded"]) == ((3, 3), (0, 23))


def test_a_failing_event_map_and_the_repeat_slice_by_hand():
    r = one([((), True), ([("S", 15, ord("c"))], False), ([("S", 16, ord("a"))], False)])   # 'a' against 'A': equal alleles
    assert (r["status"], r["variation"], r["out"]) == (EV.ALLELES, 0, [])
    r = one([((), True), ([("D", 3, 12)], False)], padded=(1005, 1039))          # a deletion from 1002: 1002 + 1 < 1005
    assert (r["status"], r["variation"], r["variant"]) == (R.REPEAT_SLICE, 0, (0, 0))
    r = one([((), True), ([("D", 5, 10)], False)], padded=(1005, 1039))          # from 1004: index 0
    assert r["status"] == 0 and r["variant"] == (1010, 1014)


def test_bases_covering_by_hand():
    g = R.get_bases_covering_ref_interval
    assert g(0, 3, b"ACTTGT", 0, P("2I4M")) == b"TTGT"            # the doc comment: a leading insertion comes before the start
    assert g(2, 3, b"ACGGTT", 0, P("2M2I2M")) == b"TT"            # an insertion AT the cut is left out
    assert g(1, 2, b"ACGGTT", 0, P("2M2I2M")) == b"CGGT"          # ... and kept inside
    assert g(0, 1, b"ACGGTT", 0, P("2M2I2M")) == b"AC"
    assert g(1, 2, b"ACT", 0, P("1M2D2M")) is None and g(0, 2, b"ACT", 0, P("1M2D2M")) is None and g(1, 3, b"ACT", 0, P("1M2D2M")) is None
    assert g(2, 2, b"ACGT", 0, P("4M")) == b"G"                   # the start test in front of the end test, one base
    assert g(2, 4, b"ACGT", 0, P("4M")) == b"GT"                  # stop one past: the test behind the loop, min(stop + 1, len)
    assert g(4, 4, b"ACGT", 0, P("4M")) == b""                    # both behind the loop: no bases
    import pytest
    with pytest.raises(R.Panic) as e:
        g(2, 5, b"ACGT", 0, P("4M"))
    assert e.value.status == R.NOT_FOUND
    with pytest.raises(R.Panic) as e:
        g(0, 1, b"ACGTA", 0, P("4M"))
    assert e.value.status == R.LENGTH
    with pytest.raises(R.Panic) as e:
        g(0, 3, b"ACGT", 0, P("2S2M"))
    assert e.value.status == R.OPERATOR


def test_trim_cigar_by_reference_by_hand():
    t = R.trim_cigar_by_reference
    assert cs(t(P("2M2I2M"), 2, 3)) == "2I2M" and cs(t(P("2M2I2M"), 0, 1)) == "2M2I"     # zero-length elements stay at both ends
    assert cs(t(P("3M2D4M"), 3, 6)) == "2M"                                              # the builder strips the deletion at the end
    assert cs(R.trim_cigar_by_bases(P("2M3I4M"), 2, 8)) == "3I4M"                        # the twin the device already has


def test_order_and_duplicates_by_hand():
    def hap(bases, is_ref=False):
        return (bases, [(R.OP_M, len(bases))], 0, (0, len(bases) - 1), is_ref)

    def go(haps, span):
        items, fates, dup = R.trim_down_haplotypes(span, haps)
        return [(t[0], i) for t, i in items], fates, dup

    # length before bytes: the shorter haplotype with larger bytes comes first
    short = (b"TTTT", P("2M1D2M"), 0, (0, 4), False)
    assert go([hap(b"AAAAA"), short], (0, 4))[0] == [(b"TTTT", 1), (b"AAAAA", 0)]
    # bytes unsigned, upper-cased: 'c' equals 'C' and folds; the first in input order represents
    assert go([hap(b"ACcA"), hap(b"ACCA"), hap(b"AACA")], (0, 3)) == ([(b"AACA", 2), (b"ACCA", 0)], [1, R.DUPLICATE, 0], [R.NONE32, 0, R.NONE32])
    # the reference wins wherever it stands in its class
    for at in range(3):
        items, fates, dup = go([hap(b"ACGT", i == at) for i in range(3)], (0, 3))
        assert items == [(b"ACGT", at)] and fates == [0 if i == at else R.DUPLICATE for i in range(3)] and dup == [R.NONE32 if i == at else at for i in range(3)]
    # haplotypes that differ only outside the span all fold
    assert go([hap(b"AACGTA"), hap(b"CACGTC"), hap(b"GACGTG")], (1, 4))[1] == [0, R.DUPLICATE, R.DUPLICATE]
    import pytest
    with pytest.raises(R.Panic) as e:
        go([(b"ACT", P("1M2D2M"), 0, (0, 4), True)], (1, 2))
    assert e.value.status == R.REF_ELIMINATED


def test_variation_present_by_hand():
    r = one([((), True), ([("S", 15, ord("A"))], False)])
    assert r["variation"] == R.VARIATION_SPAN | R.VARIATION_SET and r["ref_hap"] in (0, 1) and [o[3] for o in r["out"]].count(True) == 1
    r = one([([("S", 15, ord("A"))], True)])          # only reference haplotypes, one with an event: a span, no variation in the set
    assert r["variation"] == R.VARIATION_SPAN and r["ref_hap"] == 0


# ---- what the GPU case sets reach -----------------------------------------------------------------------------------------------------
def test_census_of_the_gpu_case_sets():
    R.REACHED.clear()
    statuses, fates = set(), set()
    sets = dict(K.sets(), exhaustive=K.exhaustive_set())
    for s in sets.values():
        o = R.trim_batch(s["regions"], s["dist"], s["padding"])
        statuses |= set(o["region_status"])
        fates |= {f if f < 0 else "rank" for f in o["hap_fate"]}
    want = {"bases:deletion_at_end", "bases:deletion_at_start", "bases:insertion_at_cut", "bases:min_len", "bases:start_behind_loop",
            "bases:stop_behind_loop", "cigar:zero_length_kept", "event:equal_key", "order:duplicate_dropped", "order:reference_replaces",
            "region:event_map_failed", "region:LOCATION", "region:LENGTH", "region:OPERATOR", "region:NOT_FOUND", "region:BUILDER", "region:REF_ELIMINATED",
            "region:REPEAT_SLICE", "span:indel", "span:none", "span:saturated", "span:snp", "trim:empty", "trim:leading", "trim:trailing", "trim:ok"}
    assert want <= R.REACHED, sorted(want - R.REACHED)
    # never reached, by construction: the STR arm; an all-insertion CIGAR with bases (a start behind the last reference base has
    # no bases: EMPTY comes first)
    assert not {"span:str", "trim:all_insertion"} & R.REACHED
    assert statuses == {0, EV.BAD_OPERATOR, EV.BLOCK, EV.CIGAR_OVERRUN, EV.ALLELES, R.LOCATION, R.LENGTH, R.OPERATOR, R.NOT_FOUND,
                        R.BUILDER, R.REF_ELIMINATED, R.REPEAT_SLICE}
    assert fates == {"rank", R.DUPLICATE, R.CUT_IN_DELETION, R.EMPTY, R.NOT_TRIMMED}
    n_haps = [len(r[4]) for s in sets.values() for r in s["regions"]]
    assert {0, 1, 2, 63, 64, 65, 128, 512} <= set(n_haps)
