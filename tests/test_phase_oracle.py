"""The restatement of the reference's reverse trim, called haplotypes and phase_calls (tests/phase_restatement.py) held to
expectations derived by hand from the cited lines -- the reference has no test of phase_calls, trim_alleles or
normalize_alleles, so the restatement is pinned by reading -- a census of what the GPU case sets (tests/phase_cases.py)
exercise, and the binding of phmm_phase_calls in the library, the header, the ctypes table and the Rust declarations.  CPU only.
Line numbers: P = src/assembly/assembly_based_caller_utils.rs, T = src/model/variant_context_utils.rs,
N = src/reads/alignment_utils.rs, G = src/haplotype/haplotype_caller_genotyping_engine.rs of the reference."""
import os
import re

import phase_cases as K
import phase_restatement as R
from lorikeet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def answer(reg, trim=True, gt=None, ploidy=2):
    """one region through the restatement, as the call's output arrays; gt: per called event its samples' genotypes"""
    if gt is not None:
        called = [ev for ev in reg["events"] if ev["call"]]
        for ev, g in zip(called, gt):
            ev["gt"] = g
    return K.expected([reg], n_samples=0 if gt is None else len(gt[0]), ploidy=ploidy, trim=trim, with_gt=gt is not None)


def test_the_export_is_in_the_library_the_binding_and_the_rust_declarations():
    lib = _lib.load()
    ffi = open(os.path.join(ROOT, "integration", "hip_ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "phmm.h")).read()
    n = "phmm_phase_calls"
    assert getattr(lib, n) is not None
    assert re.search(r"pub fn %s\s*\(" % n, ffi) and re.search(r"\bint %s\(" % n, header)
    args = next(a for name, _, a in _lib.SYMBOLS if name == n)
    decl = re.search(r"pub fn phmm_phase_calls\s*\(([^)]*)\)", ffi, re.S).group(1)
    c_decl = re.search(r"\bint phmm_phase_calls\(([^)]*)\)", header, re.S).group(1)
    assert len(args) == len([x for x in decl.split(",") if x.strip()]) == len(c_decl.split(",")) == 33
    for name in ("NO_TRIM", "ABORTED", "GT_01", "GT_10"):
        value = int(re.search(r"#define PHMM_PH_%s \(?(-?\d+)u?\)?" % name, header).group(1))
        assert getattr(_lib, "PHMM_PH_" + name) == value, name
        assert re.search(r"pub const PHMM_PH_%s: \w+ = %d;" % (name, value), ffi), name
    import tools.source_hash as SH
    assert SH.KERNEL_SOURCES["phase"] == ("phmm_phase_internal.hpp", "phmm_phase_kernels.hip")
    assert "phase=%s" % SH.source_hash("phase") in lib.phmm_build_info().decode()
    import lorikeet_amd
    assert lorikeet_amd.phase_calls is lorikeet_amd.phase.phase_calls


# ---- phase_calls ---------------------------------------------------------------------------------------------------------------
def test_two_snps_on_the_same_haplotype_are_one_group():
    # haplotype 0 is the reference, haplotype 1 carries both SNPs: S0 = S1 = {1}, total = 1 (P:1114-1120).  i = 0, j = 1:
    # |S0| == |S1| and S1 within S0 (P:1163-1167) -> together; neither is mapped, so group 0 with 0|1 and 0|1 (P:1191-1194).
    # The group's first call leads it and its start is PS (P:1025-1028).
    x = answer(K.two_snps_on_one_haplotype())
    assert x["phase_n_haps"].tolist() == [1, 1] and x["region_alt_haps"].tolist() == [1]
    assert x["phase_group"].tolist() == [0, 0] and x["phase_gt"].tolist() == [0, 0]
    assert x["phase_leader"].tolist() == [0, 0] and x["phase_set"].tolist() == [100, 100]
    assert x["region_phase_flags"].tolist() == [0] and x["hap_in_call"].tolist() == [0, 1, 0, 1]


def test_two_snps_on_the_two_alt_haplotypes_are_apart():
    # S0 = {0}, S1 = {1}, total = 2.  Not together: S1 is not within S0 and |S1| = 1 != 2.  |S0| + |S1| == total and the
    # intersection is empty (P:1208-1217) -> apart: i gets 0|1 and j 1|0 (P:1228-1235).
    x = answer(K.two_snps_on_the_two_alt_haplotypes())
    assert x["region_alt_haps"].tolist() == [2]
    assert x["phase_group"].tolist() == [0, 0] and x["phase_gt"].tolist() == [0, 1]
    assert x["phase_set"].tolist() == [100, 100]


def test_later_calls_join_through_i_with_its_phase_and_with_the_flipped_one():
    # S = {0}, {1}, {1}, {0}, total = 2.  i = 0: j = 1 apart -> group 0, 0|1 / 1|0.  j = 2: apart from call 0, which is mapped now,
    # and call 2 is not: it joins with the flipped phase of 0|1, 1|0 (P:1237-1252).  j = 3: together with call 0: it joins with
    # call 0's phase 0|1 (P:1202-1207).  i = 1 and i = 2 meet mapped calls only: nothing.
    # The flip of a 1|0 (P:1245-1249's else arm) needs an unmapped j apart from an i that holds 1|0; then S_j equals the set of an
    # earlier member with 0|1, which met j as its own i before.  No input reaches that arm, and the census does not ask for it.
    x = answer(K.joins_in_both_directions())
    assert x["phase_group"].tolist() == [0, 0, 0, 0] and x["phase_gt"].tolist() == [0, 1, 1, 0]
    assert x["phase_leader"].tolist() == [0, 0, 0, 0]


def test_a_comp_on_all_alt_haplotypes_is_together_with_everything():
    # S0 = {0}, S1 = {0, 1}, total = 2: the sizes differ, the middle clause is false (its set is empty, P:1147 and P:1198-1199),
    # comp_is_on_all_alt_haps (P:1160-1161, P:1173) -> together: 0|1 / 0|1.
    x = answer(K.on_all_alt_haplotypes())
    assert x["phase_n_haps"].tolist() == [1, 2]
    assert x["phase_group"].tolist() == [0, 0] and x["phase_gt"].tolist() == [0, 0]


def test_a_mapped_comp_met_by_an_unmapped_call_clears_the_region():
    # S = {0}, {1}, {0, 1, 2}, total = 3.  i = 0: j = 1 is neither together nor apart (1 + 1 != 3); j = 2 is on all alt haplotypes ->
    # group 0 with calls 0 and 2.  i = 1 is unmapped: j = 2 is together with it and already mapped -> the mapping is cleared and
    # the function returns (P:1176-1183): nothing in the region is phased.
    x = answer(K.abort())
    assert x["phase_group"].tolist() == [-1, -1, -1] and x["phase_gt"].tolist() == [0, 0, 0]
    assert x["phase_leader"].tolist() == [-1, -1, -1] and x["phase_set"].tolist() == [-1, -1, -1]
    assert x["region_phase_flags"].tolist() == [1] and x["region_alt_haps"].tolist() == [3]
    assert x["phase_n_haps"].tolist() == [1, 1, 3]          # the sets themselves stay reported


def test_multi_allelic_span_del_only_and_non_ref_calls_get_the_empty_set():
    # P:1282 with P:1330-1348: A / C / G has two site-specific alts, A / * and A / <NON_REF> none: the empty set each, and the
    # two SNPs around them phase with each other as if they were not there.
    x = answer(K.unmapped_calls())
    assert x["phase_n_haps"].tolist() == [1, 0, 0, 0, 1]
    assert x["phase_group"].tolist() == [0, -1, -1, -1, 0] and x["phase_leader"].tolist() == [0, -1, -1, -1, 0]
    assert x["phase_set"].tolist() == [100, -1, -1, -1, 100]


def test_the_trimmed_alt_matches_the_event_map_and_the_untrimmed_one_does_not():
    # The locus at 200 merges a deletion ACG -> A (haplotype 1) and a SNP A -> T (haplotype 2) into ACG / A / TCG.  The call
    # drops the deletion: ACG / TCG has 2 alleles against the merged 3, so it is trimmed (G:482-488).  normalize_alleles: G == G,
    # C == C leave the end, A != T stops both loops (N:608-622); no range is empty: rev_trim = 2, A / T, end = 200 (T:1063-1066).
    # Haplotype 2's event at 200 has the alt T: S = {2}.  The SNP at 210 is on haplotypes 1 and 2: S = {1, 2} = total -> together.
    x = answer(K.deletion_and_snp())
    assert x["call_rev_trim"].tolist() == [2, 0] and x["call_end"].tolist() == [200, 210]
    assert x["phase_n_haps"].tolist() == [1, 2] and x["hap_in_call"].tolist() == [0, 0, 1, 0, 1, 1]
    assert x["phase_group"].tolist() == [0, 0] and x["phase_gt"].tolist() == [0, 0]
    # with every allele kept the call is not trimmed; it has two site-specific alts anyway.  And the two-allele call with the
    # trim turned off compares TCG with T: no haplotype
    assert answer(K.deletion_and_snp(drop_deletion=False))["phase_n_haps"].tolist() == [0, 2]
    x = answer(K.deletion_and_snp(), trim=False)
    assert x["call_rev_trim"].tolist() == [0, 0] and x["call_end"].tolist() == [202, 210] and x["phase_n_haps"].tolist() == [0, 2]
    assert x["phase_group"].tolist() == [-1, -1]


def test_the_position_in_the_call_keys_the_merged_map():
    # G:394-405: the call ACG / TCG keeps the merged alleles {0, 2}; allele_mapper.remove(&idx) runs for idx = 0 and 1, the merged
    # reference and the deletion.  Haplotype 2, which carries the SNP, is not called, so S is empty although its event map holds
    # T at 200.  In deletion_and_snp the SNP at 210 calls haplotype 2 (it is allele 1 of two there).
    before = R.CENSUS["called: position-as-key differs from the merged index"]
    x = answer(K.position_as_key())
    assert R.CENSUS["called: position-as-key differs from the merged index"] == before + 1
    assert x["call_rev_trim"].tolist() == [2] and x["phase_n_haps"].tolist() == [0] and x["region_alt_haps"].tolist() == [0]


def trimmed(alleles, start=10):
    vc = R.reverse_trim_alleles(R.VariantContext(start, start + len(alleles[0]) - 1, [R.Allele(a, k == 0) for k, a in enumerate(alleles)]))
    return [a.bases for a in vc.alleles], vc.start, vc.end


def test_reverse_trim_alleles():
    # T:961-968: an allele of length 1 that is not symbolic -- '*' is one -- returns the context as it is
    assert trimmed([b"ACG", b"A"]) == ([b"ACG", b"A"], 10, 12)
    assert trimmed([b"ACG", b"TCG", b"*"]) == ([b"ACG", b"TCG", b"*"], 10, 12)
    assert trimmed([b"ACG"]) == ([b"ACG"], 10, 12)
    # AC / CAC: C == C, A == A leave the end and AC is empty (N:608-614, min_size 0); the forward loop does not run, start_trim
    # is 0: restore_one_base_at_end (T:993-1002), one base goes: A / CA
    assert trimmed([b"AC", b"CAC"]) == ([b"A", b"CA"], 10, 10)
    # AC / ACC: C == C leaves the end, A != C stops; forward A == A (N:616-622) empties the range of AC: start_trim 1, so
    # restore_one_base_at_start, which trim_forward == false never uses (T:1011): end_trim 1 stays, A / AC
    assert trimmed([b"AC", b"ACC"]) == ([b"A", b"AC"], 10, 10)
    # a symbolic allele is left out of the sequences and kept (T:970-981, T:1040-1043)
    assert trimmed([b"ACG", b"TCG", b"<NON_REF>"]) == ([b"A", b"T", b"<NON_REF>"], 10, 10)
    # nothing in common at the end: as it is
    assert trimmed([b"ACG", b"ACT"]) == ([b"ACG", b"ACT"], 10, 12)
    # The third loop of normalize_alleles (N:626-636) runs with max_shift 0 whenever the forward loop moved the start, and its
    # last_base_on_right_is_same is the test that ended the first loop with ranges left: it never moves anything here.
    assert R.CENSUS["normalize: the shift loop moved"] == 0


def test_the_calls_of_the_trim_region():
    x = answer(K.trims())
    assert x["call_rev_trim"].tolist() == [0, 1, 1, 2, 0] and x["call_end"].tolist() == [302, 310, 320, 330, 342]
    assert x["phase_n_haps"].tolist() == [1, 1, 1, 1, 1] and x["phase_group"].tolist() == [0] * 5


def test_phase_vc_reverses_a_het_whose_indexed_allele_is_not_site_specific():
    # joins_in_both_directions: calls 0 and 3 hold 0|1 (alt_allele_index 1), calls 1 and 2 hold 1|0 (index 0) (P:1062-1067).
    # Sample genotypes in index form: [0, 1] is Het; with 0|1 alleles[1] is the alt, site-specific: kept; with 1|0 alleles[0] is
    # the reference: reversed to [1, 0].  [1, 1] and [0, 0] are Hom, [-1, -1] a no-call, [-1, 1] Mixed: never reversed.
    gt = [[[0, 1], [1, 1]], [[0, 1], [-1, -1]], [[0, 0], [-1, 1]], [[0, 1], [0, 1]]]
    x = answer(K.joins_in_both_directions(), gt=gt)
    assert x["gt_phased"].tolist() == [[[0, 1], [1, 1]], [[1, 0], [-1, -1]], [[0, 0], [-1, 1]], [[0, 1], [0, 1]]]
    assert x["is_phased"].tolist() == [[1, 1]] * 4
    # ploidy 1 is never Het and never indexes (the && of P:1064); ploidy 3 with 1|0: [0, 0, 1] has the reference at index 0
    x = answer(K.joins_in_both_directions(), gt=[[[1]], [[1]], [[0]], [[-1]]], ploidy=1)
    assert x["gt_phased"].tolist() == [[[1]], [[1]], [[0]], [[-1]]]
    # and [0, 1, 1] with 0|1 the alt at index 1
    x = answer(K.joins_in_both_directions(), gt=[[[0, 1, 1]], [[0, 0, 1]], [[0, 1, 1]], [[1, 1, 1]]], ploidy=3)
    assert x["gt_phased"].tolist() == [[[0, 1, 1]], [[1, 0, 0]], [[1, 1, 0]], [[1, 1, 1]]]
    # an unphased call keeps its genotypes and is not phased
    x = answer(K.abort(), gt=[[[0, 1]], [[0, 1]], [[0, 1]]])
    assert x["gt_phased"].tolist() == [[[0, 1]]] * 3 and x["is_phased"].tolist() == [[0]] * 3


def test_the_gpu_case_sets_reach_every_branch():
    """A census over exactly what tests/test_phase_hip.py runs: a case set that stops exercising a branch fails here."""
    R.CENSUS.clear()
    for n_samples, ploidy in K.GT_SHAPES:
        for name, regions in K.sets():
            K.expected(K.draw_gt(regions, n_samples, ploidy, seed=n_samples * 10 + ploidy), n_samples, ploidy, True, True)
    K.expected([K.deletion_and_snp()], trim=False)
    want = ("link: together", "link: together by |Sj| == total alone", "link: apart", "link: unrelated", "link: empty set", "link: abort",
            "link: new group", "link: join with i's phase", "link: join with the flipped phase", "link: both mapped",
            "mapping: several site-specific alts", "mapping: no site-specific alt", "mapping: '*' in an unmapped call",
            "mapping: <NON_REF> in an unmapped call", "mapping: a trimmed allele matched",
            "called: position-as-key differs from the merged index", "trim: one allele or an allele of length 1",
            "trim: restore_one_base_at_end", "trim: restore_one_base_at_start", "trim: a symbolic allele kept", "trim: bases left the end",
            "gt: het reversed", "gt: het kept", "gt: hom", "gt: no-call", "gt: ploidy 1", "gt: ploidy 2", "gt: ploidy 3")
    missing = [k for k in want if not R.CENSUS[k]]
    assert not missing, missing
    # the seeded regions alone reach the four relations
    R.CENSUS.clear()
    K.expected([K.seeded(s) for s in K.SEEDS])
    assert all(R.CENSUS[k] for k in ("link: together", "link: apart", "link: unrelated", "link: empty set", "link: abort")), R.CENSUS


def test_pack_and_unpack_are_inverse():
    for name, regions in K.sets():
        regions = K.draw_gt(regions, 2, 2, seed=3)
        a = K.pack(regions, 2, 2, True)
        back = K.unpack(a, a["call_allele_off"], a["call_allele"], a["gt"])
        for r, b in zip(regions, back):
            assert r["haps"] == b["haps"], name
            for x, y in zip(r["events"], b["events"]):
                assert {k: x[k] for k in ("start", "alleles", "hap_allele", "call")} == {k: y[k] for k in ("start", "alleles", "hap_allele", "call")}, name
                assert not x["call"] or x["gt"] == y["gt"], name
