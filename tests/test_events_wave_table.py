"""What tests/test_events_wave_hip.py crosses, counted on the CPU from the inputs and the restatement alone
(tests/events_wave_cases.py): second and later trips of the 64-lane loops of events_hap_kernel, events_region_kernel and
events_locus_kernel, and per-locus lists of more than 64 and 128 entries.  Every count is above 0 on the new sets and 0 on the
sets of tests/events_cases.py (but for the bytes of two MNPs, see ALLELE_BYTES), each witness holds a restated result that a
loop which stopped after its first trip could not have given, and the loops restated here are read out of the source text: when
one is rewritten, the case list needs another look.  No GPU."""
import os
import re

import events_cases as K
import events_restatement as R
import events_wave_cases as W
import test_events_oracle as oracle
from conftest import ROOT
from lorikeet_amd import _lib

CSRC = os.path.join(ROOT, "lorikeet_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constant(text, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)u?\s*;" % re.escape(name), text)
    assert m, name
    return int(m.group(1))


def test_the_restated_loops_are_the_sources():
    kernels, internal = _source("phmm_events_kernels.hip"), _source("phmm_events_internal.hpp")
    assert W.LANES == 64 and "__launch_bounds__(64) void events_hap_kernel" in kernels
    assert "__launch_bounds__(64) void events_region_kernel" in kernels and "__launch_bounds__(64) void events_locus_kernel" in kernels
    once = ("for (uint64_t i = lane; i < len; i += 64) bad |= !regular(hap[ap + i]);",
            "for (uint64_t i = lane; i <= len; i += 64) bad |= !regular(ref[ref_pos - 1 + i]);",
            "for (uint32_t i = lane; i < rest_len; i += 64)",
            "for (uint32_t u = lane; u < nu && !same; u += 64)",
            "for (uint32_t a = lane; a < na + 1 && !same; a += 64)",
            "for (uint32_t a = 0; a < na && idx < 0; ++a)",
            "for (uint32_t i = lane; i < n; i += 64) p.allele_bases[at + i] = V.byte(e, pool, star, i);",
            "return i < ev->alt_len ? pool[ev->alt_off + i] : upper(ref_at_loc[ev->ref_len + (i - ev->alt_len)]);")
    for line in once:
        assert kernels.count(line) == 1, line
    assert kernels.count("for (uint32_t w = lane; w < n_words; w += 64)") == 2      # the bitmap: cleared, then read
    assert kernels.count("for (uint32_t hl = lane; hl < nh; hl += 64)") == 2        # overlapping events, the allele mapper
    assert "__shared__ uint32_t bits[EV_MAX_REF / 32], pref[EV_MAX_REF / 32 + 1];" in kernels
    assert _constant(internal, "EV_OVERLAP") == 3
    assert _constant(internal, "EV_MAX_HAPS") == _lib.PHMM_EVENTS_MAX_HAPS == W.MAX_HAPS == 512
    assert _constant(internal, "EV_MAX_REF") == _lib.PHMM_EVENTS_MAX_REF == 16384
    # downstream: the byte-by-byte comparison the chain test feeds alts of 65 and 71 bytes
    assert "for (uint32_t i = 0; in && i < len; ++i) in = p.hap_event_alt[b0 + i] == alt_bases[i];" in _source("phmm_phase_kernels.hip")


def add(total, c):
    for k, v in c.items():
        total[k] += v


def test_census_of_the_wave_sets_and_of_the_first_suite():
    total = dict.fromkeys(W.COUNTS, 0)
    by_set = {}
    for name, regions in W.SETS.items():
        by_set[name] = W.census([rg for _, rg in regions()])
        add(total, by_set[name])
    print("\nthe wave sets: %d regions" % len(W.new_regions()))
    for k in W.COUNTS:
        print("  %-66s %6d" % (k, total[k]))
        assert total[k] > 0, k
    old = dict.fromkeys(W.COUNTS, 0)
    for _, rg, dists in K.singles():
        for d in dists:
            add(old, W.census([rg], d))
    for _, rg, o in K.multis():
        add(old, W.census([rg], o.get("dist", 0), o.get("include_spanning", True), o.get("margin", 2)))
    for _, regions, d in K.random_batches():
        add(old, W.census(regions, d))
    for k in W.COUNTS:
        if k not in W.ALLELE_BYTES:
            assert old[k] == 0, (k, old[k])
    # M65_dense and M129_dense at distance 3: the reference and the alt of one MNP each, and nothing else of that length
    assert [old[k] for k in W.ALLELE_BYTES] == [0, 2, 2]
    # each set is there for counts of its own
    assert all(by_set["long_elements"][k] > 0 for k in W.COUNTS[:4] + W.ALLELE_BYTES)
    assert by_set["tail_past_64"][W.COUNTS[11]] == 2
    assert all(by_set["many_alleles"][k] > 0 for k in W.COUNTS[4:8]) and by_set["many_alleles"][W.COUNTS[6]] == 3
    assert by_set["many_distinct_haplotypes"][W.COUNTS[5]] == 3 and by_set["many_distinct_haplotypes"][W.COUNTS[7]] > 256
    assert by_set["wide_reference"][W.COUNTS[12]] == 9 + 7 and by_set["wide_reference"][W.COUNTS[13]] == 2


def events_of(r):
    alt = [b - a for a, b in zip(r["hap_event_alt_off"], r["hap_event_alt_off"][1:])]
    return list(zip(r["hap_event_ref_length"], alt))


def test_long_elements_are_what_they_claim():
    names = [n for n, _ in W.long_elements()]
    for n in (63, 64, 65, 128, 129, 200):
        assert "I%d" % n in names
    for n in (63, 64, 65, 127, 128, 130):
        assert "D%d" % n in names
    for name, rg in W.long_elements():
        r = W.restated("long_elements", name)
        assert r["region_status"] == [0], name
        assert events_of(r) == W.EXPECT[name] and len(r["event_loc"]) == len(W.EXPECT[name]), (name, events_of(r))
        assert rg["haps"][0][2] == 2 and rg["haps"][0][1][0] == (R.OP_M, 20) and rg["haps"][0][1][-1] == (R.OP_M, 20), name
    block = W.restated("long_elements", "snp_then_I70")
    assert block["hap_event_type"] == [R.SNP] and block["hap_event_start"] == [100 + W.ANCHOR]
    assert W.restated("long_elements", "I70_then_D70")["hap_event_end"] == [100 + W.ANCHOR + 70]
    assert W.restated("long_elements", "D70_then_I70")["hap_event_start"] == [100 + W.ANCHOR, 100 + W.ANCHOR + 70]


def test_a_base_that_is_not_regular_behind_the_first_trip_decides():
    """each N case has no event and its clean twin has one; the two differ in that one base alone"""
    cases = dict(W.long_elements())
    assert sorted(W.TWIN) == ["D100_N_at_70", "D63_last_base_N", "D64_last_base_N", "I70_N_at_63", "I70_N_at_64"]
    for name, twin in W.TWIN.items():
        assert W.restated("long_elements", name)["event_loc"] == [] and W.restated("long_elements", name)["hap_event_start"] == [], name
        assert len(W.restated("long_elements", twin)["event_loc"]) == 1, twin
        a, b = cases[name], cases[twin]
        differ = [i for i, (x, y) in enumerate(zip(a["ref"], b["ref"])) if x != y]
        hap_differ = [i for i, (x, y) in enumerate(zip(a["haps"][0][0], b["haps"][0][0])) if x != y]
        assert a["haps"][0][1] == b["haps"][0][1] and len(differ) + len(hap_differ) == 1, name
        if differ:   # the index the kernel's loop gives that reference base: ref[ref_pos - 1 + i], ref_pos - 1 the anchor
            at = differ[0] - W.ANCHOR
            assert a["ref"][differ[0]] == ord("N") and at == dict(D63_last_base_N=63, D64_last_base_N=64, D100_N_at_70=70)[name]
            assert at <= a["haps"][0][1][1][1]
        else:        # hap[ap + i], ap the 20 bases of the leading M
            assert a["haps"][0][0][hap_differ[0]] == ord("N") and hap_differ[0] - 20 == int(name[-2:])


def test_the_tail_behind_a_long_alt():
    for name, n_ins, n_del in (("I70_beside_D100", 70, 100), ("I64_beside_D64", 64, 64)):
        rg, ins = W.tail_region(n_ins, n_del)
        assert rg == W.named("tail_past_64", name)
        r = W.restated("tail_past_64", name)
        loc = W.ANCHOR
        assert r["region_status"] == [0] and r["event_loc"] == [100 + loc, 100 + loc + 31] and r["vc_end"][0] == 100 + loc + n_del
        off = r["allele_bases_off"]
        alleles = [bytes(r["allele_bases"][a:b]) for a, b in zip(off, off[1:])]
        assert r["event_allele_off"] == [0, 3, 6] and r["allele_kind"] == [0, 0, 0, 0, 0, 1]
        ref = rg["ref"]
        assert alleles[0] == ref[loc:loc + n_del + 1] and len(alleles[0]) == n_del + 1
        alt = ref[loc:loc + 1] + ins
        assert alleles[1] == alt + ref[loc + 1:loc + n_del + 1] and len(alleles[1]) == n_ins + 1 + n_del   # byte for byte
        assert alleles[2] == ref[loc:loc + 1]
        assert r["event_hap_allele"] == [1, 2, 0, 1, 2, 0]   # the SNP inside the deletion: the deletion's haplotype is '*'


def test_two_alts_that_differ_behind_the_first_trip_alone():
    r = W.restated("tail_past_64", "I70_twice_differing_at_68")
    assert r["region_status"] == [0] and r["allele_length"] == [1, 71, 71] and r["event_hap_allele"] == [1, 2, 0]
    a, b = bytes(r["allele_bases"][1:72]), bytes(r["allele_bases"][72:143])
    assert [i for i in range(71) if a[i] != b[i]] == [69] and bytes(r["hap_event_alt"]) == a + b


def test_repeats_behind_64_unique_events_add_no_allele():
    for n in W.MANY:
        rg = W.many_alleles_region(n)
        assert rg == W.named("many_alleles", "%d_insertions" % n) and len(rg["haps"]) == n + 3
        r = W.restated("many_alleles", "%d_insertions" % n)
        without = R.discover([dict(rg, haps=rg["haps"][:n] + rg["haps"][-1:])])
        repeats = 2 if n == 150 else 0
        assert r["region_status"] == [0] and len(r["event_loc"]) == 1 and r["event_allele_off"] == [0, n + 1 - repeats], n
        for k in ("allele_length", "allele_bases", "allele_bases_off", "event_allele_off"):
            assert r[k] == without[k], (n, k)
        m = r["event_hap_allele"]
        first = min(70, n - 1)
        assert rg["haps"][n] == rg["haps"][first] and rg["haps"][n + 1] == rg["haps"][5]
        assert m[n] == m[first] and m[n + 1] == m[5] == 6 and m[n + 2] == 0 and (first >= 64) == (n >= 65)
        if n == 150:   # haplotypes 0, 50 and 100 carry the same G
            assert m[0] == m[50] == m[100] == 1 and m[first] == first and sorted(set(m[:n])) == list(range(1, 149))
        else:
            assert m[:n] == list(range(1, n + 1))
        assert r["allele_length"] == [1] + [2 + h for h in range(n) if not (n == 150 and h in (50, 100))]


def test_two_events_that_give_one_allele_behind_64_others():
    r = W.restated("many_alleles", "equal_alleles_behind_70")
    assert r["region_status"] == [0] and r["event_allele_off"] == [0, 72] and r["allele_length"][0] == 4 and r["allele_length"][-1] == 3
    assert bytes(r["allele_bases"][:4]) == b"AGGG" and bytes(r["allele_bases"][-3:]) == b"AGG"
    assert r["event_hap_allele"] == list(range(1, 71)) + [71, 71, 0]
    assert events_of(r)[-2:] == [(2, 1), (4, 3)]     # AG -> A and AGGG -> AGG: two events, one merged allele


def test_every_haplotype_another_one():
    for name, n_haps, most in (("512_haplotypes", 512, 161), ("130_haplotypes", 130, 45)):
        r = W.restated("many_distinct_haplotypes", name)
        counts = [b - a for a, b in zip(r["event_allele_off"], r["event_allele_off"][1:])]
        assert r["region_status"] == [0] and len(r["event_loc"]) == 45 and max(counts) == most, (name, max(counts))
        assert len(r["event_hap_allele"]) == 45 * n_haps and -1 not in r["event_hap_allele"]
        assert len({(b, tuple(c), s) for b, c, s in W.named("many_distinct_haplotypes", name)["haps"]}) == min(n_haps, 480)
    m = W.restated("many_distinct_haplotypes", "512_haplotypes")["event_hap_allele"][:512]
    assert max(m) == 160 and m[0] == m[480] == 1 and [m[h] for h in (3, 192, 195, 477)] == [2, 65, 66, 160]


def test_loci_in_the_second_and_third_pass_of_the_bitmap():
    whole, cut = W.restated("wide_reference", "whole_window"), W.restated("wide_reference", "window_2048_4095")
    assert whole["event_loc"] == [W.WIDE_START + s for s in W.WIDE_SNPS]
    assert cut["event_loc"] == [W.WIDE_START + s for s in W.WIDE_SNPS if 2048 <= s <= 4095] and len(cut["event_loc"]) == 7
    assert sorted({s // 32 for s in W.WIDE_SNPS}) == [62, 63, 64, 65, 126, 127, 128]
    assert whole["event_hap_allele"] == [1, 1, 1, 0] * 6
    assert len(W.named("wide_reference", "whole_window")["ref"]) == 4300 > 2 * 64 * 32


def test_the_restatement_still_passes_the_recorded_cases():
    """tests/golden/event_map_cases.json through the restatement, as tests/test_events_oracle.py asks it"""
    oracle.test_mnps_rows()
    oracle.test_get_overlapping_events_rows()
    oracle.test_make_blocks_rows()
    oracle.test_active_haplotypes_and_event_mapper_rows()
    oracle.test_window_and_widening()
