"""phmm_trim_regions on the MI355X behind the first 256 bytes of compare(), with the first failing event map and the first trim
panic at haplotype 64 and later, with a class whose members lie in three trips and with more regions than the scan has threads,
against the restatement (tests/region_trim_restatement.py) with the claim of tests/test_region_trim_hip.py: EQUALITY on every array
of trim.OUTPUTS, the arrays filled with 0xAB before the call and untouched behind what was written.  It is all integers and bytes,
there is no tolerance.  The sets come from tests/region_trim_wave_cases.py; tests/test_region_trim_wave_table.py counts on the CPU
what they cross and shows by witnesses that a loop cut short would not have given these results."""
import numpy as np
import pytest

import events_restatement as EV
import region_trim_restatement as R
import region_trim_wave_cases as W
from lorikeet_amd import trim
from lorikeet_amd.engine import HipPairHMMEngine
from test_region_trim_hip import run, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = HipPairHMMEngine()
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(W.SETS))
def test_equals_the_restatement(eng, name):
    s = W.SETS[name]()
    same(run(eng, s, fill=0xAB), s["regions"], s["dist"], s["padding"], name)


def test_the_witnesses_by_name(eng):
    """what tests/test_region_trim_wave_table.py derives for the restatement, asked of the device itself"""
    s = W.late_difference()
    got = run(eng, s)
    ho = got["inputs"]["region_hap_off"]
    fates = {name: got["hap_fate"][ho[g]:ho[g + 1]].tolist() for g, name in enumerate(s["names"])}
    for k in W.LATE_BYTES:
        assert sorted(fates["first_difference_at_%d" % k]) == [0, 1, 2], k
    assert fates["opposite_signs_at_70_and_200"] == [0, 1] and fates["opposite_signs_at_70_and_200_reversed"] == [1, 0]
    assert fates["differences_at_200_and_300"] == [1, 0] and fates["differences_at_200_and_300_reversed"] == [0, 1]
    assert fates["lower_case_folds_at_300"] == [0, trim.FATE_DUPLICATE, 1] and fates["lower_case_folds_at_300_lower_first"] == [0, trim.FATE_DUPLICATE]
    assert not np.isin(got["out_hap_bases"], np.frombuffer(b"acgt", np.uint8)).any()
    s = W.late_class()
    got = run(eng, s)
    for g, name in enumerate(s["names"]):
        refs = W.CLASS_REFS[name]
        rep = refs[-1] if refs else 3
        f, d = got["hap_fate"][301 * g:301 * (g + 1)], got["hap_dup_of"][301 * g:301 * (g + 1)]
        assert np.flatnonzero(f == trim.FATE_DUPLICATE).tolist() == [i for i in W.CLASS_AT if i != rep], name
        assert all(d[i] == rep for i in W.CLASS_AT if i != rep) and got["out_region_ref_hap"][g] == (f[rep] if refs else -1), name
    code = dict(ALLELES=EV.ALLELES, BAD_OPERATOR=EV.BAD_OPERATOR, BLOCK=EV.BLOCK, CIGAR_OVERRUN=EV.CIGAR_OVERRUN, LENGTH=trim.STATUS_LENGTH,
                LOCATION=trim.STATUS_LOCATION, OPERATOR=trim.STATUS_OPERATOR, NOT_FOUND=trim.STATUS_NOT_FOUND,
                REF_ELIMINATED=trim.STATUS_REF_ELIMINATED)
    for s in (W.late_event_failure(), W.late_panic()):
        got = run(eng, s)
        nh = len(s["regions"][0][4])
        for g, name in enumerate(s["names"]):       # the first family in the name is the first in input order
            want = 0 if name.startswith("healthy") else code[name.split("_at_")[0]]
            assert got["region_status"][g] == want, name
            if want:
                assert np.all(got["hap_fate"][nh * g:nh * (g + 1)] == trim.FATE_NOT_TRIMMED), name
                assert got["out_region_hap_off"][g] == got["out_region_hap_off"][g + 1] and got["out_region_ref_hap"][g] == -1, name


def test_a_batch_against_each_of_its_regions_alone(eng):
    """the four late sets and many_regions(1025) in one call: equal to the restatement, two runs byte-identical, and every
    region of the late sets -- with the regions around the 1024th -- byte for byte what it gives in a call of its own"""
    regions, names = W.batch()
    s = dict(regions=regions, dist=0, padding=W.K.DEFAULT)
    first = run(eng, s, fill=0xAB)
    same(first, regions, 0, W.K.DEFAULT, "batch")
    again = run(eng, s, fill=0xAB)
    for out, _ in trim.OUTPUTS:
        assert first[out].tobytes() == again[out].tobytes(), out
    ho, oo = first["inputs"]["region_hap_off"], first["out_region_hap_off"]
    n_late = sum(len(W.SETS[k]()["regions"]) for k in W.LATE)
    assert n_late < 1024 < len(regions)
    for g in list(range(n_late)) + [n_late, 1023, 1024, 1025, len(regions) - 1]:
        alone = run(eng, s, [regions[g]])
        for out, _ in trim.REGION_OUTPUTS + (("out_region_ref_hap", None),):
            assert first[out][g:g + 1].tobytes() == alone[out].tobytes(), (names[g], out)
        for out in ("hap_fate", "hap_dup_of"):
            assert first[out][ho[g]:ho[g + 1]].tobytes() == alone[out].tobytes(), (names[g], out)
        for out in ("out_hap_start_wrt_ref", "out_hap_source", "out_hap_is_ref"):
            assert first[out][oo[g]:oo[g + 1]].tobytes() == alone[out].tobytes(), (names[g], out)
        b0, b1 = first["out_hap_off"][oo[g]], first["out_hap_off"][oo[g + 1]]
        c0, c1 = first["out_hap_cigar_off"][oo[g]], first["out_hap_cigar_off"][oo[g + 1]]
        assert first["out_hap_bases"][b0:b1].tobytes() == alone["out_hap_bases"].tobytes(), names[g]
        assert first["out_hap_cigar"][c0:c1].tobytes() == alone["out_hap_cigar"].tobytes(), names[g]
        assert np.array_equal(first["out_hap_off"][oo[g]:oo[g + 1] + 1] - b0, alone["out_hap_off"]), names[g]
        assert np.array_equal(first["out_hap_cigar_off"][oo[g]:oo[g + 1] + 1] - c0, alone["out_hap_cigar_off"]), names[g]
    assert R.DUPLICATE == trim.FATE_DUPLICATE
