"""The restatement of the reference's k-mer stage in front of the read-threading graph (tests/assembly_kmers_restatement.py)
held to the reference's own test literals (tests/golden/assembly_kmer_cases.json) and to expectations derived by hand from the
cited lines, one per quirk; a census of what the GPU case sets (tests/assembly_kmers_cases.py) exercise; and the binding of
phmm_assembly_kmers in the library, the header, the ctypes table and the Rust declarations.  CPU only.
Line numbers: R = src/read_threading/read_threading_graph.rs, A = src/read_threading/read_threading_assembler.rs of the reference."""
import os
import re

import pytest

import assembly_kmers_cases as K
import assembly_kmers_restatement as R
from lorikeet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU, TH, ST, FI = R.NON_UNIQUE, R.THREADED, R.THREAD_START, R.FIRST
NO = R.NO_ID


def test_the_export_is_in_the_library_the_binding_and_the_rust_declarations():
    lib = _lib.load()
    ffi = open(os.path.join(ROOT, "integration", "hip_ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "phmm.h")).read()
    n = "phmm_assembly_kmers"
    assert getattr(lib, n) is not None
    assert re.search(r"pub fn %s\s*\(" % n, ffi) and re.search(r"\bint %s\(" % n, header)
    args = next(a for name, _, a in _lib.SYMBOLS if name == n)
    decl = re.search(r"pub fn %s\s*\(([^)]*)\)" % n, ffi, re.S).group(1)
    c_decl = re.search(r"\bint %s\(([^)]*)\)" % n, header, re.S).group(1)
    assert len(args) == len([x for x in decl.split(",") if x.strip()]) == len(c_decl.split(",")) == 22
    for name in ("MAX_K_VALUES", "MAX_K", "MAX_REF_BASES", "MAX_READ_BASES", "MAX_POSITIONS", "REF_SHORT", "REF_NON_UNIQUE", "LOW_COMPLEXITY",
                 "KMER_NON_UNIQUE", "KMER_THREADED", "KMER_THREAD_START", "KMER_FIRST"):
        value = int(re.search(r"#define PHMM_ASM_%s (\d+)u?\b" % name, header).group(1))
        assert getattr(_lib, "PHMM_ASM_" + name) == value, name
        assert re.search(r"pub const PHMM_ASM_%s: \w+ = %d;" % (name, value), ffi), name
    assert (R.REF_SHORT, R.REF_NON_UNIQUE, R.LOW_COMPLEXITY) == (_lib.PHMM_ASM_REF_SHORT, _lib.PHMM_ASM_REF_NON_UNIQUE, _lib.PHMM_ASM_LOW_COMPLEXITY)
    assert (NU, TH, ST, FI) == (_lib.PHMM_ASM_KMER_NON_UNIQUE, _lib.PHMM_ASM_KMER_THREADED, _lib.PHMM_ASM_KMER_THREAD_START, _lib.PHMM_ASM_KMER_FIRST)
    backend = open(os.path.join(ROOT, "integration", "hip_backend.rs")).read()
    assert "pub fn assembly_kmers(" in backend and "phmm_assembly_kmers(" in backend
    import tools.source_hash as SH
    assert SH.KERNEL_SOURCES["asm"] == ("phmm_asm_internal.hpp", "phmm_asm_kernels.hip")
    assert "asm=%s" % SH.source_hash("asm") in lib.phmm_build_info().decode()
    import lorikeet_amd
    assert lorikeet_amd.assembly_kmers is lorikeet_amd.assembly.assembly_kmers


# ---- the reference's own literals ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["test_non_unique_middle", "test_read_creation_non_unique"])
def test_the_non_unique_sets_of_the_references_tests(name):
    import json
    want = json.load(open(K.GOLDEN))[name]["non_unique"]
    reg, k = K.golden()[name]
    _, g, _ = R.create_graph(reg["ref"], reg["reads"], k)
    assert g.non_unique_kmers == {w.encode() for w in want}
    x = R.region(reg["ref"], reg["reads"], k)
    assert x["n_non_unique"] == len(want)


@pytest.mark.parametrize("recover", [True, False])
@pytest.mark.parametrize("name", ["test_ref_creation", "test_ref_non_unique_creation", "test_starts_in_middle"])
def test_the_linear_cases_are_one_chain_that_spells_the_reference(name, recover):
    # assert_linear_graph simplifies the raw graph to ONE vertex that spells the reference: the raw graph is one chain.  The
    # reference's TestAssembler threads with recover_dangling_branches off; the chain is the same with the default
    reg, k = K.golden()[name]
    _, g, _ = R.create_graph(reg["ref"], reg["reads"], k, recover_dangling_branches=recover)
    assert R.chain(g) == reg["ref"]
    assert len(g.vertices) == len(reg["ref"]) - k + 1


def test_a_read_with_an_n_anywhere_adds_no_branch():
    # test_Ns_in_reads_are_not_used_for_graph: 100 reads, each the all-A reference with one N; at k = 25 every run of 25 or more
    # holds only the k-mer A^25, which is non-unique: nothing of a read is a start, the graph stays the reference's
    reg, k = K.golden()["test_Ns_in_reads_are_not_used_for_graph"]
    _, g, count = R.create_graph(reg["ref"], reg["reads"], k)
    assert g.non_unique_kmers == {b"A" * 25} and len(g.kmer_to_vertex_map) == 0
    assert count == sum((i >= 25) + (99 - i >= 25) for i in range(100))
    x = R.region(reg["ref"], reg["reads"], k)
    assert all(not (f & (TH | ST)) for fl in x["read_flags"] for f in fl)
    assert x["flags"] == R.REF_NON_UNIQUE | R.LOW_COMPLEXITY


# ---- one quirk each, derived by hand ------------------------------------------------------------------------------------------
def test_the_scan_from_zero_puts_a_kmer_with_a_low_quality_base_into_the_set():
    # R:125 `for i in 0..=stop_position`: the run is [2, 11) but the loop starts at 0.  ACGACGTTGCA: ACG at 0 (its C is the
    # low-quality base) and ACG at 3 -> non-unique, although the run itself holds ACG once.  find_start (R:575) runs over
    # 2 .. 8: GAC at 2 is not non-unique.  thread_sequence visits 2 ..= 8 (R:538).  The reference's seven 3-mers are unrelated.
    x = R.region(*_rq(K.scan_from_zero()), 3)
    assert (x["flags"], x["n_sequences"], x["n_non_unique"], x["n_tracked"], x["n_distinct"]) == (0, 2, 1, 7 + 6, 7 + 8)
    assert x["read_flags"] == [[FI | NU, FI, FI | TH | ST, NU | TH, FI | TH, FI | TH, FI | TH, FI | TH, FI | TH, 0, 0]]
    assert x["read_ids"] == [[7, 8, 9, 7, 10, 11, 12, 13, 14, NO, NO]]
    assert x["ref_flags"] == [FI | TH | ST] + [FI | TH] * 6 + [0, 0] and x["ref_ids"] == list(range(7)) + [NO, NO]


def test_the_exclusive_bound_leaves_a_run_whose_only_unique_kmer_is_its_last_without_a_start():
    # R:573-575 `for i in start..stop.saturating_sub(k)`: AAAAC at k = 3 tries 0 and 1, both AAA (non-unique, R:131-132); AAC at
    # 2 is unique but never tried -> None, thread_sequence does nothing (R:488-490).  The run still counts (R:383).
    x = R.region(*_rq(K.only_the_last_kmer_is_unique()), 3)
    assert (x["flags"], x["n_sequences"], x["n_non_unique"], x["n_tracked"], x["n_distinct"]) == (0, 2, 1, 7, 9)
    assert x["read_flags"] == [[FI | NU, NU, FI, 0, 0]]


def test_a_reference_of_exactly_k_bases_threads_nothing():
    # find_start returns Some(0) (R:570-571); R:492 `sequence.len() <= start_pos + kmer_size`: 3 <= 0 + 3 -> return.  No vertex,
    # an empty map; 0 * 4 > 0 is false (R:262).  One base fewer is A:935-938.
    x = R.region(*_rq(K.reference_of_exactly_k()), 3)
    assert (x["flags"], x["n_sequences"], x["n_non_unique"], x["n_tracked"], x["n_distinct"]) == (0, 1, 0, 0, 1)
    assert x["ref_flags"] == [FI | ST, 0, 0]
    y = R.region(b"AC", [], 3)
    assert y["flags"] == R.REF_SHORT and y["n_sequences"] == y["n_distinct"] == 0 and y["ref_flags"] == [0, 0]


def test_a_duplicate_of_the_reference_source_kmer_does_not_grow_the_map():
    # The reference ACGTTGCA enters its six 3-mers.  TACGT: TAC is new (R:602, R:636-637: 7 entries).  ACG: TAC has no edge out;
    # get_kmer_vertex(ACG, false) is None because ACG is the reference source (R:614-615); create_vertex (R:756) and track_kmer
    # finds it there already (R:636): an eighth vertex, still 7 entries.  CGT merges into the mapped vertex (R:758).
    reg = K.duplicate_of_the_reference_source()
    _, g, _ = R.create_graph(reg["ref"], reg["reads"], 3)
    assert len(g.kmer_to_vertex_map) == 7 and len(g.vertices) == 8 and g.vertices.count(b"ACG") == 2
    x = R.region(reg["ref"], reg["reads"], 3)
    assert x["n_tracked"] == 7 and x["n_distinct"] == 7 and x["read_flags"] == [[FI | TH | ST, TH, TH, 0, 0]]


def test_quality_one_below_the_minimum_splits_a_read_and_the_minimum_does_not():
    # R:402 `qual >= min`: qualities 10 10 9 10 10.  At min 10 two runs of exactly k = 2: each counts (R:364 `len >= k`), and
    # neither has a start: 0 .. 2 - 2 and 3 .. 5 - 2 are empty ranges (R:575).  At min 9 one run of five: start 0, visits 0 ..= 3.
    reg = K.quality_at_the_threshold()
    x, y = R.region(reg["ref"], reg["reads"], 2, 10), R.region(reg["ref"], reg["reads"], 2, 9)
    assert x["n_sequences"] == 3 and y["n_sequences"] == 2
    # (GT at 2 is not FIRST: the reference GATTCCAGT ends in it)
    assert x["read_flags"] == [[FI, FI, 0, FI, 0]] and y["read_flags"] == [[FI | TH | ST, FI | TH, TH, FI | TH, 0]]


def test_n_and_lower_case_n_are_both_unusable_and_bytes_compare_with_their_case():
    # R:401 `base.to_ascii_uppercase() != b'N'`: ACnGT and ACNGT are two runs each, ACcGT is one.  Kmer compares the bytes as they
    # are: Cc and cG are new k-mers beside CN / Cn.
    x = R.region(*_rq(K.lower_and_upper_n()), 2)
    assert x["n_sequences"] == 1 + 2 + 2 + 1
    assert x["read_flags"][2] == [TH | ST, FI | TH, FI | TH, TH, 0]          # AC and GT were seen in the first read


def test_the_low_complexity_threshold_is_strict():
    # R:262 `non_unique.len() * 4 > map.len()`.  AAAAC: AAA is non-unique (and the reference's own: A:940-956), AAC is tracked.
    # CGTAG adds three tracked k-mers: 4 > 4 is false.  CGTA adds two: 4 > 3.
    x, y = R.region(*_rq(K.on_the_threshold()), 3), R.region(*_rq(K.one_over_the_threshold()), 3)
    assert (x["n_non_unique"], x["n_tracked"], x["flags"]) == (1, 4, R.REF_NON_UNIQUE)
    assert (y["n_non_unique"], y["n_tracked"], y["flags"]) == (1, 3, R.REF_NON_UNIQUE | R.LOW_COMPLEXITY)


def _rq(reg):
    return reg["ref"], reg["reads"]


# ---- what the GPU sets reach ---------------------------------------------------------------------------------------------------
def test_the_gpu_case_sets_reach_every_branch():
    n = K.census(K.calls().values())
    assert all(v > 0 for v in n.values()), n


def test_the_layout_of_the_expected_arrays_with_and_without_windows():
    # the read plane runs over the bases as given: a window's planes lie at its place, the rest is 0 and NO_ID
    reg = K.region(K.UNRELATED_REF, [K.read("TTACGACGTTGCATT", low=(3,))])
    cut = K.region(K.UNRELATED_REF, [K.read("ACGACGTTGCA", low=(1,))])
    a, b = K.expected(K.call([reg], [3]), windows=[[(2, 11)]]), K.expected(K.call([cut], [3]))
    assert a["read_kmer_flags"][0].tolist() == [0, 0] + b["read_kmer_flags"][0].tolist() + [0, 0]
    assert a["read_kmer_id"][0].tolist() == [NO, NO] + b["read_kmer_id"][0].tolist() + [NO, NO]
    assert a["n_tracked"].tolist() == b["n_tracked"].tolist() == [[13]]
