"""phmm_assembly_regions on the MI355X past the first trip of its 64-lane loops, with scans of more than one entry a thread and
with positions past 2^32, against the restatement (tests/assembly_regions_restatement.py) with the claim of
tests/test_assembly_regions_hip.py: EQUALITY on every output array and on required, NaN compared as NaN, the arrays filled with
0xAB before the call.  There is no tolerance: region_density and read_mean_qual are one correctly rounded division each.  The
cases come from tests/assembly_regions_wave_cases.py; tests/test_assembly_regions_wave_table.py counts on the CPU what they cross
and shows by witnesses that a loop cut short would not have given these results."""
import numpy as np
import pytest

import assembly_regions_wave_cases as W
from lorikeet_amd import _lib
from lorikeet_amd.engine import HipPairHMMEngine, PhmmError
from test_assembly_regions_hip import W as A
from test_assembly_regions_hip import call, same

pytestmark = pytest.mark.gpu
ALONE = sorted(n for n in W.CASES if n != "together")


@pytest.fixture(scope="module")
def eng():
    e = HipPairHMMEngine()
    yield e
    e.close()


@pytest.mark.parametrize("name", ALONE)
def test_equals_the_restatement(eng, name):
    a, p = W.case(name)
    same(call(eng, a, p, fill=0xAB), W.restated(name), name)


def test_the_witnesses_by_name(eng):
    """what tests/test_assembly_regions_wave_table.py derives for the restatement, asked of the device itself"""
    for lead in (0, 37):
        r = 1 if lead else 0
        states = [int(call(eng, *W.case("cut_active_%d_lead%d" % (n, lead)))["region_states"][r]) for n in (4099, 4100, 4102)]
        assert states == [4099, 4100, 4100], (lead, states)
        states = [int(call(eng, *W.case("cut_inactive_%d_lead%d" % (n, lead)))["region_states"][r]) for n in (4100, 4101, 4102, 4300)]
        assert states == [4100] * 4, (lead, states)
    for name, e in (("one_minimum_4090", 4091), ("one_minimum_70", 71), ("equal_100_and_4000", 4001), ("equal_64_apart", 75),
                    ("equal_4096_apart", 4099), ("nan_behind_end", 201), ("nan_4097_beside_200", 4097), ("none", 4100)):
        assert call(eng, *W.case("cut_site_" + name))["region_states"][0] == e, name
    for n in (65, 130):
        got = call(eng, *W.case("cigar_%d_elements" % n))
        reached = got["region_reads"].tolist()
        assert 0 in reached and 1 not in reached and 2 not in reached, n
    for n in W.MEMBER_SIZES:
        got = call(eng, *W.case("members_%d" % n))
        assert np.diff(got["region_read_off"].astype(np.int64)).tolist() == [n, n // 2 + 3]
    got = call(eng, *W.case("positions_past_2_32"))
    assert int(got["region_end"][-1]) == W.P62 - 2 and int(got["region_padded_end"][-1]) == W.P62 - 1
    assert any(int(s) < W.P32 <= int(e) for s, e in zip(got["region_start"], got["region_end"]))


def test_together_and_each_of_its_parts_alone(eng):
    """read_cases()["two_windows"] and the new parts in one call: equal to the restatement, two runs byte-identical, each part's
    share byte for byte what the part gives in a call of its own under the same parameters"""
    a, p = W.case("together")
    whole = call(eng, a, p, fill=0xAB)
    same(whole, W.restated("together"), "together")
    again = call(eng, a, p, fill=0xAB)
    for name, _ in A.OUTPUTS:
        assert whole[name].tobytes() == again[name].tobytes(), name
    parts, _ = W.together_parts()
    S = int(a["n_samples"])
    k0 = r_reads = 0
    for tag, part in parts:
        alone = call(eng, part, p, fill=0xAB)
        same(alone, W.restate(part, p), tag)
        k1 = k0 + len(part["profile_len"])
        r0, r1 = int(whole["profile_region_off"][k0]), int(whole["profile_region_off"][k1])
        assert alone["required"][0] == r1 - r0 > 0, tag
        assert whole["profile_status"][k0:k1].tobytes() == alone["profile_status"].tobytes(), tag
        assert (whole["profile_region_off"][k0:k1 + 1] - np.uint32(r0)).tobytes() == alone["profile_region_off"].tobytes(), tag
        for name, _ in A.REGION_OUTPUTS:
            assert whole[name][r0:r1].tobytes() == alone[name].tobytes(), (tag, name)
        offs = whole["region_read_off"][r0 * S:r1 * S + 1]
        m0, m1 = int(offs[0]), int(offs[-1])
        assert alone["required"][1] == m1 - m0 > 0, tag
        assert (offs - np.uint32(m0)).tobytes() == alone["region_read_off"].tobytes(), tag
        assert (whole["region_reads"][m0:m1] - np.uint32(r_reads)).tobytes() == alone["region_reads"].tobytes(), tag
        n_reads = len(part["read_pos"])
        assert whole["read_mean_qual"][r_reads:r_reads + n_reads].tobytes() == alone["read_mean_qual"].tobytes(), tag
        k0, r_reads = k1, r_reads + n_reads
    assert k0 == len(a["profile_len"]) and r_reads == len(a["read_pos"])


def test_the_capacity_protocol_where_a_scan_thread_takes_three_entries(eng):
    """scan_pairs_2049: capacities (0, 0) give the two sizes and write nothing else, the exact capacities give the result"""
    a, p = W.case("scan_pairs_2049")
    want = W.restated("scan_pairs_2049")
    R_, M_ = (int(x) for x in want["required"])
    assert R_ * int(a["n_samples"]) == 2049 and M_ > 2049
    with pytest.raises(PhmmError) as e:
        call(eng, a, p, capacity=(0, 0), fill=0xAB)
    assert e.value.code == _lib.PHMM_ERR_EVENT_CAPACITY and list(e.value.required) == [R_, M_]
    for name, arr in e.value.outputs.items():
        assert name == "required" or np.all(arr.view(np.uint8) == 0xAB), name
    same(call(eng, a, p, capacity=(R_, M_), fill=0xAB), want, "exact")
    with pytest.raises(PhmmError) as e:
        call(eng, a, p, capacity=(R_, M_ - 1), fill=0xAB)
    assert e.value.code == _lib.PHMM_ERR_EVENT_CAPACITY and list(e.value.required) == [R_, M_]
