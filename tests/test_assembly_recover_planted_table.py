"""The planted graphs of tests/assembly_recover_planted_cases.py on the CPU: the builders hand the restatement exactly the planted
strings, the oracle gives the reference's asserted LeadingInDel CIGAR on family C's strings, FLOOR passes the host's rule where it
is used, and the families together reach every rule of the aligner that the census names.  This proves the cases, not the kernel:
tests/test_assembly_recover_planted_hip.py runs them on the device."""
import re

import pytest

import assembly_prune_restatement as P
import assembly_recover_planted_cases as PC
import assembly_recover_restatement as R
from oracle import oracle


@pytest.fixture(scope="module")
def census():
    return PC.census(PC.groups())


def test_the_families_have_the_sizes_the_cases_file_states():
    count = lambda f, k=None: len({id(m) for g in PC.family(f) for m in g["members"] if k in (None, m["k"])})  # noqa: E731
    assert count("A") == 900 + 14 + 12 and len(PC.family("A")) == 9 + 2 * 9
    assert count("B", 1) == 2 * 14 * 14 and count("B", 3) == 56 * 56 == 3136 and len(PC.family("B")) == 2 * (48 + 8)
    assert count("C") == 2 * (9 + 3 + 2) and len(PC.family("C")) == 4
    assert count("D", 1) == 2 * len(PC.d_pairs()) and count("D", 11) == 15 + 2 and len(PC.family("D")) == 6
    names = [g["name"] for g in PC.groups()]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("family", PC.FAMILIES)
def test_the_restatement_aligns_the_planted_strings(family):
    """one end of the planted kind per graph; whenever the restatement aligns, end_ref_len / end_alt_len are the planted lengths,
    and get_bases_for_path on the restatement's own paths returns the planted bytes.  Where the prune factor lies above every edge
    find_path drops the alt path (R:1667-1677): a tail is then too short, and a head arrives with the join vertex's byte alone"""
    seen = set()
    for g in PC.family(family):
        for m in g["members"]:
            x = PC.answer(m, g["cfg"])
            tail = m["kind"] == R.TAIL
            assert (x["n_tails"], x["n_heads"]) == ((1, 0) if tail else (0, 1)) and x["end_kind"] == [m["kind"]], PC.describe(m, g["cfg"])
            dropped = m["factor"] > 0
            if x["end_status"][0] == R.TOO_SHORT:
                want_len = 1 if dropped else len(m["alt"]) - (0 if tail else m["k"] - 1)   # the alt path's vertices
                least = max(1, g["cfg"].min_dangling_branch_length) if tail else g["cfg"].min_dangling_branch_length
                assert want_len < least + 1 and x["end_ref_len"][0] == 0, PC.describe(m, g["cfg"])
                continue
            assert x["end_status"][0] not in (R.NO_PATH, R.LOOP, R.AT_REF_END), PC.describe(m, g["cfg"])
            assert x["end_ref_len"] == [len(m["ref"])] and x["end_alt_len"] == [1 if dropped else len(m["alt"])], PC.describe(m, g["cfg"])
            if id(m) in seen:
                continue
            seen.add(id(m))
            gr = R.Graph(m["k"], m["graph"]["kmers"], m["graph"]["edges"])
            end = x["end_vertex"][0]
            if tail:
                _, alt_path = R.find_path_upwards_to_lowest_common_ancestor(gr, end, m["factor"])
                ref_path = R.get_reference_path(gr, alt_path[0], True, R.get_heaviest_edge(gr, alt_path[1], False))
            else:
                _, alt_path = R.find_path_downwards_to_highest_common_descendant_of_reference(gr, end, m["factor"])
                ref_path = R.get_reference_path(gr, alt_path[0], False, None)
            assert R.get_bases_for_path(gr, ref_path, not tail) == m["ref"], PC.describe(m, g["cfg"])
            assert R.get_bases_for_path(gr, alt_path, not tail) == (m["alt"][:1] if dropped else m["alt"]), PC.describe(m, g["cfg"])
            assert not P.has_cycles(gr)
    assert seen


def test_the_oracle_on_the_references_own_strings():
    """where the golden case's strategy is LeadingInDel the oracle gives the reference's asserted CIGAR on the strings without
    the shared byte; of the other cases only the pair is reused.  With the shared byte in front the planted graph's end aligns
    those strings: a match more"""
    pairs = PC.golden_pairs()
    assert len(pairs) == 14
    asserted = [c for _, _, _, c in pairs if c is not None and c["strategy"] == "LeadingInDel"]
    assert len(asserted) == 1
    for c in asserted:
        cig, off = oracle.sw_align(c["reference"], c["read"], c["params"], "LeadingInDel")
        assert (off, oracle.cigar_to_string(cig)) == (c["expected_offset"], c["expected_cigar"]), c["source"]
        w = next(name for name, v in PC.NAMED.items() if list(v) == c["params"])
        g = next(g for g in PC.family("C") if g["weights"] == w)
        for m in g["members"]:
            if m["note"] == c["source"]:
                x = PC.answer(m, g["cfg"])
                assert (m["ref"], m["alt"]) == (b"G" + c["reference"].encode(), b"G" + c["read"].encode())
                assert PC.cigar_string(x["end_cigar"][0][:x["end_n_cigar"][0]]) == "1M3D5M", PC.describe(m, g["cfg"])   # 3D5M behind the shared byte
    for g in PC.family("C"):
        assert [(m["ref"][1:].decode(), m["alt"][1:].decode()) for m in g["members"][::2]] == [(r, a) for _, r, a, _ in pairs]


def test_floor_passes_the_hosts_rule_where_it_is_used_and_nowhere_larger():
    used = [g for g in PC.groups() if g["weights"] == "FLOOR"]
    assert sorted((g["family"], g["k"]) for g in used) == [("A", 1), ("B", 1), ("B", 3)]
    for g in used:
        assert PC.floor_is_accepted(g["graphs"])
        slab_len = max(len(x["kmers"]) for x in g["graphs"]) + g["k"] + 2
        assert 20000000 * (2 * slab_len + 2) < 10 ** 9 and slab_len <= 23
    assert not PC.floor_is_accepted([PC.tail_graph(b"G" + b"A" * 10, b"G" + b"C" * 10)])          # 23 vertices: L = 26
    assert not any(PC.floor_is_accepted(g["graphs"]) for g in PC.family("D"))


def test_the_floor_decides_where_the_cases_file_says_so():
    """the oracle's CIGAR on FLOOR_DECIDES is the one the floor gives, not the one the unclamped sums would give: a kernel
    without the clamp cannot pass family A under FLOOR"""
    g = next(g for g in PC.family("A") if g["weights"] == "FLOOR")
    for ref, alt, with_floor, without in PC.FLOOR_DECIDES:
        assert with_floor != without
        assert oracle.cigar_to_string(oracle.sw_align(ref, alt, PC.FLOOR, "LeadingInDel")[0]) == with_floor, (ref, alt)
        m = next(m for m in g["members"] if (m["ref"], m["alt"]) == (ref, alt))
        x = PC.answer(m, g["cfg"])
        assert PC.cigar_string(x["end_cigar"][0][:min(4, x["end_n_cigar"][0])]) == "".join(re.findall(r"\d+[MID]", with_floor)[:4])


@pytest.mark.parametrize("name", PC.CENSUS)
def test_the_families_reach(census, name):
    """every count above 0; the failure names nothing, the census names the first case that reaches each count"""
    assert name in census and census[name][0] > 0, name
    assert census[name][1]


def test_which_family_reaches_what(census):
    """the rules the issue found reached by accident or not at all, each by the family built for it"""
    assert set(census) == set(PC.CENSUS)
    first = lambda name: census[name][1].split("-")[0]  # noqa: E731
    assert first("floor") == "A" and "FLOOR" in census["floor"][1]
    assert "FREE_GAPS" in census["dropped trailing D"][1] and "FREE_GAPS" in census["dropped trailing D behind four or more elements"][1]
    assert first("a gap over 64 in the CIGAR") == "D" and first("head: cannot extend") == "D"
    assert first("extension by k > 1 vertices") == "B" and first("a head that min_dangling_branch_length = 1 refuses") == "B"
    only_d = PC.census(PC.family("D"))
    for name in ("backtrack_over_64", "a gap over 64 in the CIGAR", "5 elements", "more than 5 elements", "leading I", "leading D",
                 "dropped trailing D behind four or more elements"):
        assert only_d[name][0] > 0, name
