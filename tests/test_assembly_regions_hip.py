"""phmm_assembly_regions on the MI355X against the restatement of pop_ready_assembly_regions and of the regions' fetch
(tests/assembly_regions_restatement.py), through the C ABI as lorikeet_amd.assembly_regions binds it.  EQUALITY on every output
array, region_density and read_mean_qual included (NaN compared as NaN): each is one correctly rounded division of exactly
representable integers, so there are no tolerances.  The cases come from tests/assembly_regions_cases.py;
tests/test_assembly_regions_oracle.py holds the restatement to the reference's own tests and to hand-derived expectations and
counts on the CPU what the cases reach.  The module imports lorikeet_amd.assembly_regions at the top: without the export every
test here fails."""
import importlib

import numpy as np
import pytest

import assembly_regions_cases as K
import assembly_regions_restatement as R
from lorikeet_amd import _lib, activity
from lorikeet_amd.engine import HipPairHMMEngine, PhmmError

W = importlib.import_module("lorikeet_amd.assembly_regions")   # (the package exports the function under the module's name)

pytestmark = pytest.mark.gpu
REGION_CASES, READ_CASES = K.region_cases(), K.read_cases()
ALL = dict(REGION_CASES, **READ_CASES)


@pytest.fixture(scope="module")
def eng():
    e = HipPairHMMEngine()
    yield e
    e.close()


def call(eng, a, p, **kw):
    return W.assembly_regions(eng, a, assembly_region_extension=p["extension"], min_region_size=p["min_region_size"],
                              max_region_size=p["max_region_size"], max_prob_propagation=p["max_prob_propagation"],
                              active_prob_threshold=p["threshold"], max_input_depth=p["max_input_depth"], **kw)


def want_of(a, p, **kw):
    return R.assembly_regions(a, p["extension"], p["min_region_size"], p["max_region_size"], p["max_prob_propagation"],
                              np.float32(p["threshold"]), p["max_input_depth"], **kw)


def same(got, want, tag):
    for name, dt in (("required", np.uint32),) + W.OUTPUTS:
        if name not in want:     # (without reads: the three arrays of part B are not written)
            assert name in ("region_read_off", "region_reads", "read_mean_qual") and len(got[name]) == 0, (tag, name)
            continue
        g, w = got[name], np.asarray(want[name], dt)
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), (tag, name, g[:16], w[:16])
    return want


@pytest.mark.parametrize("name", sorted(ALL))
def test_equals_the_restatement(eng, name):
    """every case in a call of its own: lists of 0 .. 129 states against maxima 1 .. 300, boundaries at bit 63 and at bit 0 of the
    second word and behind one pass of 64 words, runs that end at the maximum, lists around max + propagation, the region at
    stop + 1, the cut site (ties, the minimum size and below, none, after a drain, the last state, NaN, infinities, min > max),
    the contig's end and the start past it, padding on both sides, 2 / 64 / 65 profiles; groups of 0 .. 130 reads, the long read
    early in its group, the four edges of the fetch, reads without reference bases or qualities, samples, the depth cap"""
    a, p = ALL[name]
    want = same(call(eng, a, p, fill=0xAB), want_of(a, p), name)
    if name == "start_past_contig":     # the status beside healthy profiles
        assert list(want["profile_status"]) == [0, W.STATUS_START_PAST_CONTIG, 0] and list(want["profile_region_off"]) == [0, 2, 5, 7]
    if name == "cut_min_above_max_reached":
        assert list(want["profile_status"]) == [W.STATUS_MIN_REGION_SIZE]
    if name in ("cut_min_above_max_not_reached", "cut_min_above_max_inactive"):
        assert list(want["profile_status"]) == [0] and want["required"][0] > 0
    if name == "one_short":
        assert want["required"][0] == 0
    if name == "start_is_stop_plus_1":
        assert int(want["region_states"].sum()) == 15      # five states stay unpopped
    if name == "depth_above_cap":
        assert want["region_flags"][0] & W.OVER_DEPTH
    if name == "long_read_early":
        assert 1 in want["region_reads"][want["region_read_off"][3]:want["region_read_off"][4]]


def test_without_the_read_arrays_part_b_is_skipped(eng):
    for name in ("two_windows", "group_of_65"):
        a, p = READ_CASES[name]
        got = call(eng, a, p, with_reads=False, fill=0xAB)
        want = want_of(a, p, with_reads=False)
        same(got, want, name)
        assert got["required"][1] == 0 and not got["region_n_reads"].any()


def test_a_profile_alone_in_a_batch_and_in_a_second_call(eng):
    """byte for byte: one profile alone, the same profile among others, and the same call again"""
    a, p = REGION_CASES["profiles_65"]
    whole = call(eng, a, p)
    again = call(eng, a, p)
    for name, _ in W.OUTPUTS:
        assert whole[name].tobytes() == again[name].tobytes(), name
    for k in (0, 17, 64):
        f, n = int(a["profile_first"][k]), int(a["profile_len"][k])
        one = dict(a, profile_prob=a["profile_prob"][f:f + n].copy(), profile_first=np.zeros(1, np.uint32),
                   **{key: a[key][k:k + 1] for key in ("profile_len", "profile_start", "profile_stop", "profile_contig_length", "profile_window")})
        alone = call(eng, one, p)
        r0, r1 = int(whole["profile_region_off"][k]), int(whole["profile_region_off"][k + 1])
        assert alone["required"][0] == r1 - r0 and alone["profile_status"][0] == whole["profile_status"][k]
        for name, _ in W.REGION_OUTPUTS:
            assert alone[name].tobytes() == whole[name][r0:r1].tobytes(), (k, name)


def test_the_chain_from_the_activity_profile(eng):
    """phmm_activity_profile's real output on a tiny window, two profiles of it, passed on as it is with its reads"""
    rng = np.random.default_rng(5)
    ref = bytes(rng.choice(list(b"ACGT"), 160).tolist())
    reads = []
    for pos in sorted(int(x) for x in rng.integers(1000, 1100, 24)):
        n = min(50, 1160 - pos)
        bases = bytearray(ref[pos - 1000:pos - 1000 + n])
        if 1060 <= pos + 10 < 1160:
            bases[10] = ord("A") if bases[10] != ord("A") else ord("C")
        reads.append((pos, [(n << 4) | 0], bytes(bases), [35] * n))
    windows = activity.pack([activity.Window(1000, ref, 5000, [reads, reads[::3]])])
    res = activity.activity_profile(eng, windows, max_prob_propagation=8, max_filter_size=8, profile_size=80)
    a = W.from_activity(res, windows, profile_size=80)
    assert list(a["profile_len"]) == list(res.profile_len) and list(a["profile_stop"]) == [1079, 1159]
    p = dict(K.DEFAULTS, extension=12, min_region_size=5, max_region_size=30, max_prob_propagation=8, max_input_depth=20)
    got = W.assembly_regions(eng, res, windows, assembly_region_extension=12, min_region_size=5, max_region_size=30, max_prob_propagation=8,
                             max_input_depth=20, profile_size=80, fill=0xAB)
    want = same(got, want_of(a, p), "chain")
    assert want["required"][0] >= 4 and want["required"][1] > 0 and (want["region_flags"] & W.ACTIVE).any()


def test_the_capacity_protocol(eng):
    a, p = READ_CASES["two_windows"]
    want = want_of(a, p)
    R_, M_ = (int(x) for x in want["required"])
    with pytest.raises(PhmmError) as e:      # all capacities 0: the sizes, nothing else
        call(eng, a, p, capacity=(0, 0), fill=0xAB)
    assert e.value.code == _lib.PHMM_ERR_EVENT_CAPACITY and list(e.value.required) == [R_, M_]
    for name, arr in e.value.outputs.items():
        assert name == "required" or np.all(arr.view(np.uint8) == 0xAB), name
    same(call(eng, a, p, capacity=(R_, M_), fill=0xAB), want, "exact")
    for cap in ((R_ - 1, M_), (R_, M_ - 1)):   # one too few: the sizes, nothing else
        with pytest.raises(PhmmError) as e:
            call(eng, a, p, capacity=cap, fill=0xAB)
        assert e.value.code == _lib.PHMM_ERR_EVENT_CAPACITY and list(e.value.required) == [R_, M_]
        for name, arr in e.value.outputs.items():
            assert name == "required" or np.all(arr.view(np.uint8) == 0xAB), (cap, name)
    got = call(eng, a, p, capacity=(R_ + 3, M_ + 5), fill=0xAB)   # more room than needed: the rest is untouched
    same(got, want, "roomy")


def test_no_profiles_and_empty_lists_are_fine(eng):
    a, p = K.make([], None)
    got = call(eng, a, p, fill=0xAB)
    assert list(got["required"]) == [0, 0] and list(got["profile_region_off"]) == [0]
    a, p = K.make([K.profile([]), K.profile([])], [[], []], n_samples=2)
    same(call(eng, a, p, fill=0xAB), want_of(a, p), "empty lists")


def bad(a, p, **edit):
    b = dict(a)
    par = dict(p)
    for k, v in edit.items():
        (par if k in par else b)[k] = v
    return b, par


INVALID = {
    "min_region_size_0": (dict(min_region_size=0), "min_region_size"),
    "max_region_size_0": (dict(max_region_size=0), "max_region_size"),
    "null_profile_len": (dict(omit=("profile_len",)), "null array"),
    "null_profile_prob": (dict(omit=("profile_prob",), n_prob=1 << 20), "null array"),
    "null_profile_status": (dict(omit=("profile_status",)), "null array"),
    "null_capacity": (dict(omit=("capacity",)), "null array"),
    "null_region_start": (dict(omit=("region_start",), capacity=(100, 1000)), "null array"),
    "null_region_reads": (dict(omit=("region_reads",), capacity=(100, 1000)), "null array"),
    "null_profile_window": (dict(omit=("profile_window",)), "null array"),
    "null_read_pos": (dict(omit=("read_pos",)), "null array"),
    "null_read_quals": (dict(omit=("read_quals",)), "null array"),
    "list_past_the_array": (lambda a: dict(profile_len=a["profile_len"] + np.array([0, 0, 40], np.uint32)), "profile 2: profile_first + profile_len"),
    "contig_length_0": (lambda a: dict(profile_contig_length=a["profile_contig_length"] * np.array([1, 0, 1], np.uint64)), "profile 1: contig length 0"),
    "window_out_of_range": (lambda a: dict(profile_window=np.array([2, 0, 3], np.uint32)), "profile 2: window 3 of 3"),
    "group_read_off_start": (lambda a: dict(group_read_off=a["group_read_off"] + np.uint32(1)), "group_read_off does not start at 0"),
    "group_read_off_order": (lambda a: dict(group_read_off=np.array([0, 80, 70, 82, 232, 232, 302], np.uint32)), "group_read_off not monotonic"),
    "read_cigar_off_start": (lambda a: dict(read_cigar_off=a["read_cigar_off"] + np.uint32(1)), "read_cigar_off does not start at 0"),
    "read_cigar_off_order": (lambda a: dict(read_cigar_off=np.concatenate([a["read_cigar_off"][:9], a["read_cigar_off"][8:9] - np.uint32(1), a["read_cigar_off"][10:]])), "read 8: read_cigar_off not monotonic"),
    "read_off_start": (lambda a: dict(read_off=a["read_off"] + np.uint32(1)), "read_off does not start at 0"),
    "read_off_order": (lambda a: dict(read_off=np.concatenate([a["read_off"][:5], a["read_off"][4:5] - np.uint32(1), a["read_off"][6:]])), "read_off not monotonic"),
    "read_pos_decreases": (lambda a: dict(read_pos=np.concatenate([a["read_pos"][:90], a["read_pos"][89:90] - 1, a["read_pos"][91:]])), "pos is smaller"),
    "read_pos_negative": (lambda a: dict(read_pos=np.concatenate([[-1], a["read_pos"][1:]])), "pos is negative"),
    "cigar_operator_9": (lambda a: dict(read_cigar=np.concatenate([a["read_cigar"][:7], [(5 << 4) | 9], a["read_cigar"][8:]]).astype(np.uint32)), "CIGAR element 7"),
    "position_beyond_2_62": (lambda a: dict(profile_start=a["profile_start"] + np.array([0, 1 << 62, 0], np.uint64)), "profile 1: position beyond 2^62"),
    "no_samples": (dict(n_samples=0), "no samples"),
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_arguments_write_nothing_and_name_the_offender(eng, name):
    a, p = READ_CASES["two_windows"]
    edit, message = INVALID[name]
    kw = {}
    if callable(edit):
        a = dict(a, **edit(a))
    else:
        kw = {k: v for k, v in edit.items() if k in ("omit", "capacity")}
        a, p = bad(a, p, **{k: v for k, v in edit.items() if k not in kw})
    with pytest.raises(PhmmError) as e:
        call(eng, a, p, fill=0xAB, **kw)
    assert e.value.code == _lib.PHMM_ERR_INVALID_ARG and message in str(e.value), str(e.value)
    for arr_name, arr in e.value.outputs.items():
        assert np.all(arr.view(np.uint8) == 0xAB), arr_name
