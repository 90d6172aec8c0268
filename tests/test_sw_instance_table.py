"""The tables tests/test_sw_instances_hip.py iterates over are the kernel source's (a newly compiled Smith-Waterman instance
fails here until the sweep covers it), the flag packing has the three shapes the kernel's backtrack expects for every listed K,
and the generated batches have the lengths that select each instance.  No GPU."""
import os
import re

import pytest

import test_sw_instances_hip as sweep

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lorikeet_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _macro_list(text, name):
    """The X(L, K) entries of `#define name(X) ...` (continuation lines included)."""
    m = re.search(r"#define\s+%s\(X\)((?:.*\\\n)*.*)\n" % re.escape(name), text)
    assert m, name
    return tuple((int(a), int(b)) for a, b in re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*\)", m.group(1)))


def _int_array(text, name):
    m = re.search(r"const\s+int\s+%s\[\]\s*=\s*\{([^}]*)\}" % re.escape(name), text)
    assert m, name
    return tuple(int(x) for x in m.group(1).split(","))


def test_the_sweep_covers_exactly_the_compiled_instances():
    text = _source("phmm_sw_kernels.hip")
    assert _macro_list(text, "PHMM_SW_LIST") == sweep.SW_LIST
    assert _macro_list(text, "PHMM_SW_LIST_T") == sweep.SW_LIST_T
    for L, name in ((16, "kSwK16"), (8, "kSwK8"), (32, "kSwK32"), (64, "kSwK64")):
        assert _int_array(text, name) == sweep.SW_K[L], name
    assert _int_array(text, "kSwK64T") == sweep.SW_K_T
    # the planner picks from the kSwK arrays, the launcher from the macro lists: they must name the same instances
    assert sorted(sweep.SW_LIST) == sorted((L, K) for L, ks in sweep.SW_K.items() for K in ks)
    assert sweep.SW_LIST_T == tuple((64, K) for K in sweep.SW_K_T)
    for ks in list(sweep.SW_K.values()) + [sweep.SW_K_T]:
        assert list(ks) == sorted(set(ks))
    assert len(sweep.SW_LIST) == 32 and len(sweep.SW_LIST_T) == 6
    # every one of them in both variants, once
    want = {(L, K, False, lite) for L, K in sweep.SW_LIST for lite in (False, True)} | {(L, K, True, lite) for L, K in sweep.SW_LIST_T for lite in (False, True)}
    assert set(sweep.CASES) == want and len(sweep.CASES) == len(want) == 76
    # the special instances are one geometry each (the wide test and the 20 000-base test assert these)
    assert "phmm_sw_align_kernel<16, 16, false, true, false>" in text and "phmm_sw_align_kernel<16, 32, false, false, true>" in text


def sw_flag_words(K):
    """phmm_sw_internal.hpp, restated: a pair of dwords (tags, gap bits) per 16 cells; a remainder of 9-15 cells takes a pair of
    its own, one of 1-8 cells ONE dword (tags in the top half, gap bits in the bottom half)."""
    full, rem = divmod(K, 16)
    return 2 * full + (0 if rem == 0 else 1 if rem <= 8 else 2)


def sw_tag_words(K):
    return (K + 15) // 16


# dwords per lane and step, K by K, written out: (flag words, tag words, shape of the remainder)
PACKING = {2: (1, 1, "shared"), 3: (1, 1, "shared"), 4: (1, 1, "shared"), 5: (1, 1, "shared"), 6: (1, 1, "shared"), 8: (1, 1, "shared"),
           10: (2, 1, "pair"), 12: (2, 1, "pair"), 14: (2, 1, "pair"), 16: (2, 1, "none"),
           19: (3, 2, "shared"), 20: (3, 2, "shared"), 22: (3, 2, "shared"), 24: (3, 2, "shared"),
           26: (4, 2, "pair"), 28: (4, 2, "pair"), 32: (4, 2, "none")}


def test_flag_packing_of_every_listed_k():
    header = _source("phmm_sw_internal.hpp")
    # the restatement above is the header's formula: a change there fails here until the shapes below are looked at again
    assert "constexpr int sw_flag_words(int K) { return 2 * (K / 16) + (K % 16 == 0 ? 0 : K % 16 <= 8 ? 1 : 2); }" in header
    assert "constexpr int sw_tag_words(int K) { return (K + 15) / 16; }" in header
    listed = sorted({K for _, K in sweep.SW_LIST} | set(sweep.SW_K_T))
    assert listed == sorted(PACKING)
    for K in listed:
        words, tags, shape = PACKING[K]
        assert (sw_flag_words(K), sw_tag_words(K)) == (words, tags), K
        rem = K % 16
        assert shape == ("none" if rem == 0 else "shared" if rem <= 8 else "pair"), K
        # four bits per cell fit; the shared dword's halves (2 bits per cell each) do not overlap
        assert 32 * words >= 4 * K and 32 * tags >= 2 * K
        if shape == "shared":
            assert 2 * rem + 2 * rem <= 32 and words == 2 * (K // 16) + 1
        # one vector store per lane and step holds them (dword ... dwordx4)
        assert 1 <= words <= 4
    # the mixes the sweep is there for: a full pair next to the shared dword, and the odd K
    assert [K for K in listed if K > 16 and PACKING[K][2] == "shared"] == [19, 20, 22, 24]
    assert [K for K in listed if K % 2] == [3, 5, 19]


@pytest.mark.parametrize("case", [c for c in sweep.CASES if not c[3]], ids=sweep.case_id)
def test_generated_batches_select_their_instance(case):
    L, K, transposed, _ = case
    kp = sweep.k_prev(L, K, transposed)
    full = L * K
    b = sweep.make_batches(L, K, transposed)
    assert b == sweep.make_batches(L, K, transposed)                      # the same batch every time
    ks = sweep.k_list(L, transposed)

    def planned_k(longest):   # phmm_sw.cpp, sw_plan: the smallest listed K whose strip covers the longest; else the largest
        return next((k for k in ks if L * k >= longest), ks[-1])

    lane_len = [sweep.laned_length(p, transposed) for p in b["main"]]
    other_len = [len(p[1]) if transposed else len(p[0]) for p in b["main"]]
    assert all(len(r) >= 1 and len(a) >= 1 for call in b.values() if call for r, a in call)
    assert L * kp < max(lane_len) <= full and max(lane_len) == full and planned_k(max(lane_len)) == K
    for need in (L * kp + 1, full - 1, full, 1, min(K + 1, full), min(L + 1, full)):
        assert need in lane_len, need
    for need in (1, 2, L - 1, L, L + 1):
        assert need in other_len, need
    assert max(other_len) >= 200
    assert len(b["main"]) % (64 // L) != 0 or L == 64                     # idle groups in the last wave
    # lanes without columns and a partly filled last lane inside the batch
    assert any(-(-x // K) < L and x % K for x in lane_len) and any(-(-x // K) <= L // 2 for x in lane_len)
    # the single alignment at the lower boundary
    assert len(b["boundary"]) == 1
    one = sweep.laned_length(b["boundary"][0], transposed)
    assert one == L * kp + 1 and planned_k(one) == K and (kp == 0 or planned_k(one - 1) == kp)
    if transposed:
        assert max(lane_len) <= 512 and b["strips"] is None               # sw_plan: the sweep along the alternate has one strip of at most 512 rows
        # alternates shorter and longer than a strip of the ordinary sweep would be
        assert min(other_len) == 1 and max(other_len) > 64 * K
    elif K == ks[-1]:
        s_len = [sweep.laned_length(p, False) for p in b["strips"]]
        for need in (full + 1, 2 * full, 2 * full + 1, full, 1):
            assert need in s_len, need
        assert max(s_len) == 2 * full + 1 and planned_k(max(s_len)) == K
        assert sweep.expected_instance(L, K, False, 0, b["strips"])["strips"] == 3
        assert len(b["strips"]) % (64 // L) != 0 or L == 64
    else:
        assert b["strips"] is None
    assert sweep.expected_instance(L, K, transposed, 0, b["main"])["strips"] == 1


def test_wide_batches_have_two_and_three_strips_within_the_wide_range():
    b = sweep.make_wide_batches()
    for name, longest, strips in (("two_strips", 300, 2), ("three_strips", 513, 3)):
        pairs = b[name]
        assert max(len(a) for _, a in pairs) == longest and sweep.expected_instance(16, 16, False, sweep.SW_WIDE, pairs)["strips"] == strips
        assert (longest - 1) % 16 != 15 or longest == 513                   # the last lane in use is partly filled (513: one column)
        assert len(pairs) % 4 != 0
        reach = max(len(r) for r, _ in pairs) + longest + 2
        for prm in sweep.WIDE_WEIGHTS:
            big = max(abs(prm.match_value), abs(prm.mismatch_penalty), abs(prm.gap_open_penalty), abs(prm.gap_extend_penalty))
            assert 100000000 <= big * reach < 1000000000                    # sw_plan: wide from 1e8, refused from 1e9
