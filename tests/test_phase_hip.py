"""phmm_phase_calls on the MI355X against the restatement of the reference's reverse trim, called haplotypes and phase_calls
(tests/phase_restatement.py), through the C ABI as lorikeet_amd.phase binds it.  EQUALITY on every output array: it is all
integers and bytes, there are no tolerances.  The regions come from tests/phase_cases.py; tests/test_phase_oracle.py holds
the restatement to hand-derived expectations and counts on the CPU what the sets exercise.  The module imports
lorikeet_amd.phase at the top: without the call every test here fails."""
import numpy as np
import pytest

import phase_cases as K
from lorikeet_amd import _lib, events, phase
from lorikeet_amd.engine import HipPairHMMEngine, PhmmError

pytestmark = pytest.mark.gpu
SETS = dict(K.sets())


@pytest.fixture(scope="module")
def eng():
    e = HipPairHMMEngine()
    yield e
    e.close()


def run(eng, regions, n_samples=0, ploidy=0, with_gt=False, **kw):
    a = K.pack(regions, n_samples, ploidy, with_gt)
    return phase.phase_calls(eng, a, a["region_hap_off"], a["call_allele_off"], a["call_allele"], a["gt"], n_samples, ploidy, **kw)


def same(res, want, tag):
    for k in phase.OUTPUTS:
        got, exp = getattr(res, k), want[k]
        if exp is None:
            assert got is None, (tag, k)
            continue
        assert got.dtype == exp.dtype and got.shape == exp.shape, (tag, k, got.dtype, got.shape, exp.shape)
        assert np.array_equal(got, exp), (tag, k, np.argwhere(got != exp)[:5].tolist(), got.reshape(-1)[:16], exp.reshape(-1)[:16])


@pytest.mark.parametrize("name", sorted(SETS))
def test_equals_the_restatement(eng, name):
    """each set in a call of its own (the hand cases: one region per call), with two samples of ploidy 2"""
    regions = K.draw_gt(SETS[name], 2, 2, seed=11)
    same(run(eng, regions, 2, 2, True, fill=0xAB), K.expected(regions, 2, 2, True, True), name)


@pytest.mark.parametrize("n_samples,ploidy", K.GT_SHAPES)
def test_everything_in_one_call(eng, n_samples, ploidy):
    """every region of every set in one call, at 1 and 3 samples and ploidy 1, 2 and 3: the census' runs"""
    regions = [r for name, regs in K.sets() for r in K.draw_gt(regs, n_samples, ploidy, seed=n_samples * 10 + ploidy)]
    same(run(eng, regions, n_samples, ploidy, True, fill=0xAB), K.expected(regions, n_samples, ploidy, True, True), (n_samples, ploidy))


def test_a_region_of_a_batch_equals_the_same_region_alone_and_a_second_call(eng):
    regions = [r for _, regs in K.sets() for r in regs]
    regions = K.draw_gt(regions, 2, 2, seed=5)
    first, again = run(eng, regions, 2, 2, True), run(eng, regions, 2, 2, True)
    for k in phase.OUTPUTS:
        assert getattr(first, k).tobytes() == getattr(again, k).tobytes(), k
    e0 = m0 = 0
    for g, reg in enumerate(regions):
        alone = run(eng, [reg], 2, 2, True)
        ne, nm = len(reg["events"]), len(reg["events"]) * len(reg["haps"])
        for k in phase.OUTPUTS:
            got, whole = getattr(alone, k), getattr(first, k)
            if k.startswith("region_"):
                part = whole[g:g + 1]
            elif k == "hap_in_call":
                part = whole[m0:m0 + nm]
            else:
                part = whole[e0:e0 + ne]
            if k == "phase_leader":
                part = np.where(part >= 0, part - e0, part)
            assert np.array_equal(got, part), (g, k)
        e0, m0 = e0 + ne, m0 + nm


def test_without_gt_without_hap_in_call_and_with_the_trim_turned_off(eng):
    regions = K.draw_gt([r for _, regs in K.sets() for r in regs], 1, 2, seed=7)
    full = run(eng, regions, 1, 2, True)
    res = run(eng, regions, fill=0xAB)
    want = K.expected(regions)
    same(res, want, "gt NULL")
    assert res.is_phased is None and res.gt_phased is None
    res = run(eng, regions, 1, 2, True, omit=("hap_in_call",))
    assert res.hap_in_call is None
    for k in phase.OUTPUTS:
        assert k == "hap_in_call" or np.array_equal(getattr(res, k), getattr(full, k)), k
    same(run(eng, regions, 1, 2, True, trim=False, fill=0xAB), K.expected(regions, 1, 2, False, True), "trim off")
    # the trim decides something in these sets: the locus of deletion_and_snp matches only when trimmed
    assert not np.array_equal(run(eng, regions, trim=False).phase_n_haps, full.phase_n_haps)


def test_empty_calls_and_regions_without_events_or_haplotypes(eng):
    res = run(eng, [])
    assert all(getattr(res, k) is None or len(getattr(res, k)) == 0 for k in phase.OUTPUTS)
    empty = dict(haps=[], events=[])
    regions = [empty, dict(haps=[[], []], events=[]), K.two_snps_on_one_haplotype(), empty, dict(haps=[], events=[K.event(5, [b"A", b"T"], [])])]
    same(run(eng, regions, fill=0xAB), K.expected(regions), "empty regions")
    same(run(eng, [empty, empty], fill=0xAB), K.expected([empty, empty]), "only empty regions")
    # samples but no ploidy-sized rows to write, and no sample at all
    regions = K.draw_gt(regions, 0, 2, seed=1)
    res = run(eng, regions, 0, 2, True)
    assert res.gt_phased.shape == (3, 0, 2) and res.phase_group.tolist() == [0, 0, -1]


def chain_regions():
    """two regions for discover_events: SNPs on three haplotypes over 60 reference bases, one of them with an insertion"""
    rng = np.random.RandomState(3)
    out = []
    for g in range(2):
        ref = bytes(rng.choice(list(b"ACGT"), 60).astype(np.uint8))
        flip = lambda b: b"ACGT"[(b"ACGT".index(b) + 1) % 4]  # noqa: E731
        def hap(at):
            h = bytearray(ref)
            for p in at:
                h[p] = flip(ref[p])
            return bytes(h)
        haps = [(ref, "60M", 0), (hap([10, 30]), "60M", 0), (hap([10, 30, 45]), "60M", 0), (hap([20]), "60M", 0)]
        if g == 1:
            h = hap([10])
            haps.append((h[:25] + b"GG" + h[25:], "25M2I35M", 0))
        out.append(events.Region(ref, 1000 * (g + 1), haps, (1000 * (g + 1) + 2, 1000 * (g + 1) + 57), 100000))
    return out


def test_the_chain_from_discover_events(eng):
    """discover_events -> hand-made call lists and GT -> phase_calls, on the arrays as they come"""
    regs = chain_regions()
    ev = events.discover_events(eng, regs, with_haplotype_events=True)
    region_hap_off = events.pack(regs)["region_hap_off"]
    n_events = len(ev.vc_start)
    assert n_events >= 7
    A = np.diff(ev.event_allele_off.astype(np.int64))
    calls = [list(range(int(a))) for a in A]
    calls[1] = []                                   # one event is not called
    n_samples, ploidy = 2, 2
    gt = np.zeros((n_events, n_samples, ploidy), np.int32)
    for e, c in enumerate(calls):
        if len(c) > 1:
            gt[e] = [[0, len(c) - 1], [len(c) - 1, len(c) - 1]]
    call_allele_off = np.concatenate([[0], np.cumsum([len(c) for c in calls])]).astype(np.uint32)
    call_allele = np.array([x for c in calls for x in c], np.uint32)
    res = phase.phase_calls(eng, ev, region_hap_off, call_allele_off, call_allele, gt, n_samples, ploidy, fill=0xAB)
    a = dict(ev._asdict(), region_hap_off=region_hap_off)
    want = K.expected(K.unpack(a, call_allele_off, call_allele, gt), n_samples, ploidy, True, True)
    same(res, want, "chain")
    assert (res.phase_group >= 0).sum() >= 4 and res.region_phase_flags.tolist() == [0, 0]


def broken(change):
    """the arrays of a small valid call with one thing wrong"""
    regions = K.draw_gt([K.deletion_and_snp(), K.joins_in_both_directions()], 1, 2, seed=2)
    a = K.pack(regions, 1, 2, True)
    change(a)
    return a


def put(key, index, value):
    def change(a):
        a[key] = a[key].copy()
        a[key][index] = value
    return change


def null(key):
    def change(a):
        a[key] = None
    return change


def many_haplotypes(a):
    a["region_hap_off"] = np.array([0, 513, 516], np.uint32)


INVALID = {
    "a required pointer is NULL (region arrays)": null("region_hap_off"),
    "a required pointer is NULL (event arrays)": null("vc_start"),
    "a required pointer is NULL (event_hap_allele)": null("event_hap_allele"),
    "a required pointer is NULL (call_allele)": null("call_allele"),
    "a required pointer is NULL (allele_bases)": null("allele_bases"),
    "a required pointer is NULL (hap_event_off)": null("hap_event_off"),
    "a required pointer is NULL (hap_event_start, hap_event_alt_off)": null("hap_event_start"),
    "a required pointer is NULL (hap_event_alt)": null("hap_event_alt"),
    "region_event_off does not start at 0": put("region_event_off", 0, 1),
    "region 1: region_event_off decreases": put("region_event_off", 1, 9),
    "region_hap_off does not start at 0": put("region_hap_off", 0, 1),
    "region 1: region_hap_off decreases": put("region_hap_off", 1, 9),
    "region 0: 513 haplotypes, more than 512": many_haplotypes,
    "event_allele_off does not start at 0": put("event_allele_off", 0, 1),
    "event 1: event_allele_off decreases": put("event_allele_off", 2, 1),
    "call_allele_off does not start at 0": put("call_allele_off", 0, 1),
    "event 1: call_allele_off decreases": put("call_allele_off", 1, 99),
    "allele_bases_off does not start at 0": put("allele_bases_off", 0, 1),
    "allele 1: allele_bases_off decreases": put("allele_bases_off", 2, 1),
    "hap_event_off does not start at 0": put("hap_event_off", 0, 1),
    "haplotype 1: hap_event_off decreases": put("hap_event_off", 1, 3),
    "hap_event_alt_off does not start at 0": put("hap_event_alt_off", 0, 1),
    "haplotype event 1: hap_event_alt_off decreases": put("hap_event_alt_off", 2, 0),
    "event 0: the call does not start with allele 0": put("call_allele", 0, 1),
    "event 0: call allele 1 is not above the one before it": put("call_allele", 1, 0),
    "event 0: call allele 1 reaches A_e (3)": put("call_allele", 1, 3),
    "allele 4: unknown kind 3": put("allele_kind", 4, 3),
    "event 1: the reference allele is not plain": put("allele_kind", 3, 1),
    "event 0: call allele 1 has length 0": put("allele_length", 2, 0),
    "event 0: call allele 1 is longer than its bytes": put("allele_length", 2, 4),
    "event 2: sample 0: gt entry 2 is outside [-1, 2)": put("gt", (2, 0, 1), 2),
    "event 1: sample 0: gt entry -2 is outside [-1, 2)": put("gt", (1, 0, 0), -2),
    "haplotype 1: its events do not ascend by start (event 1)": put("hap_event_start", 1, 200),
    "haplotype 2: its events do not ascend by start (event 1)": put("hap_event_start", 3, 150),
}


def call(eng, a, n_samples=1, ploidy=2, **kw):
    return phase.phase_calls(eng, a, a["region_hap_off"], a["call_allele_off"], a["call_allele"], a["gt"], n_samples, ploidy, fill=0xAB, **kw)


@pytest.mark.parametrize("message", sorted(INVALID))
def test_invalid_arguments_are_named_and_nothing_is_written(eng, message):
    with pytest.raises(PhmmError) as err:
        call(eng, broken(INVALID[message]))
    assert err.value.code == _lib.PHMM_ERR_INVALID_ARG
    assert message in str(err.value), str(err.value)
    for k, v in err.value.outputs.items():
        assert np.all(np.frombuffer(v.tobytes(), np.uint8) == 0xAB), k
    # the call still works afterwards
    assert call(eng, broken(lambda a: None)).phase_group.tolist() == [0, 0, 0, 0, 0, 0]


def test_invalid_arguments_that_are_not_arrays(eng):
    good = broken(lambda a: None)
    for kw, message in ((dict(ploidy=0), "ploidy is 0 with gt given"),
                        (dict(omit=("is_phased",)), "a required pointer is NULL (gt without is_phased or gt_phased)"),
                        (dict(omit=("gt_phased",)), "a required pointer is NULL (gt without is_phased or gt_phased)"),
                        (dict(omit=("phase_set",)), "a required pointer is NULL (event arrays)"),
                        (dict(omit=("region_alt_haps",)), "a required pointer is NULL (region arrays)")):
        with pytest.raises(PhmmError) as err:
            call(eng, good, **kw)
        assert err.value.code == _lib.PHMM_ERR_INVALID_ARG and message in str(err.value), str(err.value)
        for k, v in err.value.outputs.items():
            assert np.all(np.frombuffer(v.tobytes(), np.uint8) == 0xAB), k
    lib = eng.lib
    z = np.zeros(8, np.uint8)
    args = [eng._h, 0] + [None] * 15 + [1, 2, None, 0] + [None] * 10
    assert lib.phmm_phase_calls(*args, z.ctypes.data_as(_lib.u8p), None) == _lib.PHMM_ERR_INVALID_ARG
    assert "is_phased or gt_phased without gt" in eng.last_error()
    args[20] = 2
    assert lib.phmm_phase_calls(*args, None, None) == _lib.PHMM_ERR_INVALID_ARG
    assert "flags holds bits outside PHMM_PH_NO_TRIM" in eng.last_error()
    args[20] = 0
    assert lib.phmm_phase_calls(*args, None, None) == _lib.PHMM_OK      # n_regions == 0
