"""phmm_discover_events on the MI355X past the first trip of its 64-lane loops and with per-locus lists of more than 64 and 128
entries, against the restatement (tests/events_restatement.py) with the claim of tests/test_events_hip.py: EQUALITY on every
array of DENSE + HAPS, on allele_bases, hap_event_alt and required.  Nothing here is floating point, so there is no tolerance.
The regions come from tests/events_wave_cases.py; tests/test_events_wave_table.py counts on the CPU what they cross."""
import numpy as np
import pytest

import events_restatement as R
import events_wave_cases as W
import phase_cases
from lorikeet_amd import _lib, events, phase
from lorikeet_amd.engine import HipPairHMMEngine, PhmmError
from test_events_hip import DENSE, check, run, same

pytestmark = pytest.mark.gpu
EVERY = [(s, name) for s, regions in W.SETS.items() for name, _ in regions()]


@pytest.fixture(scope="module")
def eng():
    e = HipPairHMMEngine()
    yield e
    e.close()


@pytest.mark.parametrize("set_name,name", EVERY, ids=["%s-%s" % e for e in EVERY])
def test_each_region_alone(eng, set_name, name):
    same(run(eng, [W.named(set_name, name)]), W.restated(set_name, name), name)


@pytest.mark.parametrize("set_name", sorted(W.SETS))
def test_each_set_in_one_call(eng, set_name):
    check(eng, [rg for _, rg in W.SETS[set_name]()], set_name)


def test_the_witnesses_by_name(eng):
    """What tests/test_events_wave_table.py derives for the restatement, asked of the device itself."""
    for name, twin in W.TWIN.items():
        assert len(run(eng, [W.named("long_elements", name)]).event_loc) == 0, name
        assert len(run(eng, [W.named("long_elements", twin)]).event_loc) == 1, twin
    for name, n_ins, n_del in (("I70_beside_D100", 70, 100), ("I64_beside_D64", 64, 64)):
        rg, ins = W.tail_region(n_ins, n_del)
        res = run(eng, [rg])
        a, b = int(res.allele_bases_off[1]), int(res.allele_bases_off[2])
        assert bytes(res.allele_bases[a:b]) == rg["ref"][W.ANCHOR:W.ANCHOR + 1] + ins + rg["ref"][W.ANCHOR + 1:W.ANCHOR + n_del + 1], name
    res = run(eng, [W.named("many_alleles", "150_insertions")])
    assert res.event_allele_off.tolist() == [0, 149] and res.event_hap_allele[150:].tolist() == [70, 6, 0]
    res = run(eng, [W.named("many_alleles", "equal_alleles_behind_70")])
    assert res.event_allele_off.tolist() == [0, 72] and res.event_hap_allele[70:].tolist() == [71, 71, 0]
    res = run(eng, [W.named("wide_reference", "whole_window")])
    assert res.event_loc.tolist() == [W.WIDE_START + s for s in W.WIDE_SNPS]


def part(res, regions, g):
    """Region g's share of a batched result in the form of R.discover([regions[g]]): offsets from 0, event_region 0."""
    nh = [len(r["haps"]) for r in regions]
    a, b = int(res.region_event_off[g]), int(res.region_event_off[g + 1])
    per_event = [nh[r] for r in res.event_region.tolist()]
    m0 = sum(per_event[:a])
    m1 = m0 + sum(per_event[a:b])
    x0, x1 = int(res.event_allele_off[a]), int(res.event_allele_off[b])
    y0, y1 = int(res.allele_bases_off[x0]), int(res.allele_bases_off[x1])
    h0 = sum(nh[:g])
    e0, e1 = int(res.hap_event_off[h0]), int(res.hap_event_off[h0 + nh[g]])
    z0, z1 = int(res.hap_event_alt_off[e0]), int(res.hap_event_alt_off[e1])
    cut = lambda k, lo, hi, base=0: [v - base for v in np.asarray(getattr(res, k))[lo:hi].tolist()]  # noqa: E731
    out = dict(region_event_off=[0, b - a], region_status=cut("region_status", g, g + 1), event_region=[0] * (b - a),
               event_allele_off=cut("event_allele_off", a, b + 1, x0), event_hap_allele=cut("event_hap_allele", m0, m1),
               allele_length=cut("allele_length", x0, x1), allele_kind=cut("allele_kind", x0, x1),
               allele_bases_off=cut("allele_bases_off", x0, x1 + 1, y0), allele_bases=bytes(res.allele_bases[y0:y1]),
               hap_event_off=cut("hap_event_off", h0, h0 + nh[g] + 1, e0), hap_event_alt_off=cut("hap_event_alt_off", e0, e1 + 1, z0),
               hap_event_alt=bytes(res.hap_event_alt[z0:z1]))
    for k in ("event_start", "event_end", "event_loc", "vc_start", "vc_end", "event_flags"):
        out[k] = cut(k, a, b)
    for k in ("hap_event_start", "hap_event_end", "hap_event_ref_length", "hap_event_type"):
        out[k] = cut(k, e0, e1)
    return out


def test_together_and_reversed(eng):
    """events_cases.multis() and every new region in one call, then the same regions reversed: equal to the restatement, each
    new region's share equal to the region run alone, two runs byte-identical."""
    regions, first = W.together()
    alone = {}
    for order in (regions, regions[::-1]):
        res = check(eng, order, "together")
        again = run(eng, order)
        for k, (a, b) in zip(res._fields, zip(res, again)):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), k
        new = range(first, len(order)) if order is regions else range(len(order) - first)
        assert len(new) == len(W.new_regions())
        for g in new:
            key = g if order is regions else len(order) - 1 - g
            if key not in alone:
                alone[key] = run(eng, [order[g]])
            same(alone[key], part(res, order, g), ("share", g))
    assert len(alone) == len(W.new_regions())


@pytest.mark.parametrize("dist", [0, 1, 3])
@pytest.mark.parametrize("spanning", [True, False])
def test_spanning_off_and_mnp_distances(eng, spanning, dist):
    for set_name in ("tail_past_64", "long_elements"):
        for name, rg in W.SETS[set_name]():
            check(eng, [rg], (name, spanning, dist), dist, spanning)
        check(eng, [rg for _, rg in W.SETS[set_name]()], (set_name, spanning, dist), dist, spanning)
    # without spanning events the SNP inside the long deletion has no '*'
    res = run(eng, [W.named("tail_past_64", "I70_beside_D100")], dist, spanning)
    assert res.allele_kind.tolist() == [0, 0, 0, 0, 0] + [1] * spanning


def test_without_haplotype_events(eng):
    for name, rg in W.many_alleles():
        full, lean = run(eng, [rg]), run(eng, [rg], maps=False)
        same(lean, W.restated("many_alleles", name), name, maps=False)
        assert lean.hap_event_off is None and lean.required[4:].tolist() == [0, 0]
        for k in DENSE + ("allele_bases",):
            assert np.asarray(getattr(full, k)).tobytes() == np.asarray(getattr(lean, k)).tobytes(), (name, k)


@pytest.mark.parametrize("set_name,name", [("many_alleles", "150_insertions"), ("many_distinct_haplotypes", "512_haplotypes")])
def test_exact_capacities(eng, set_name, name):
    rg, want = W.named(set_name, name), W.restated(set_name, name)
    need = [len(want["event_region"]), len(want["allele_length"]), len(want["allele_bases"]), len(want["event_hap_allele"]),
            len(want["hap_event_start"]), len(want["hap_event_alt"])]
    assert run(eng, [rg]).required.tolist() == need and need[1] > 128 and all(need)
    same(run(eng, [rg], capacity=need, fill=0xA5), want, "exact")
    for k in (1, 2, 3):
        cap = list(need)
        cap[k] -= 1
        with pytest.raises(PhmmError) as err:
            run(eng, [rg], capacity=cap, fill=0xA5)
        assert err.value.code == _lib.PHMM_ERR_EVENT_CAPACITY and err.value.required.tolist() == need, (k, err.value.required)
        for field, arr in err.value.outputs.items():
            if field != "required":
                assert np.all(arr.view(np.uint8) == 0xA5), (k, field)
    same(run(eng, [rg], capacity=need, fill=0xA5), want, "exact again")


def test_the_chain_into_phasing(eng):
    """discover_events -> hand-made call lists and GT -> phmm_phase_calls on the arrays as they come: alleles of 101 and 171
    bytes through reverse_trim (the first call drops its last allele, the deletion), alts of 71 and 201 bytes through
    phase_match_kernel's byte-by-byte comparison, and an alt that differs from the call's in byte 69 alone.  phmm_phase_calls
    documents no limit on an allele's length, and refuses none of these."""
    regs = [W.named("tail_past_64", "I70_beside_D100"), W.named("tail_past_64", "I64_beside_D64"), W.named("many_alleles", "65_insertions"),
            W.named("long_elements", "I200"), W.named("long_elements", "I70_then_D70"), W.named("tail_past_64", "I70_twice_differing_at_68")]
    ev = run(eng, regs)
    same(ev, R.discover(regs), "chain")
    region_hap_off = events.pack(regs)["region_hap_off"]
    A = np.diff(ev.event_allele_off.astype(np.int64)).tolist()
    assert A == [3, 3, 3, 3, 66, 2, 2, 3]
    calls = [list(range(a)) for a in A]      # every call keeps all of its alleles ...
    calls[0] = [0, 1]                        # ... but this one: reference (101 bytes) and the insertion (171), 100 to trim
    calls[7] = [0, 2]                        # and this: haplotype 0 is called, and its alt is the call's but for byte 69 of 71
    n_samples, ploidy = 2, 2
    gt = np.zeros((len(A), n_samples, ploidy), np.int32)
    for e, c in enumerate(calls):
        gt[e] = [[0, len(c) - 1], [len(c) - 1, len(c) - 1]]
    call_allele_off = np.concatenate([[0], np.cumsum([len(c) for c in calls])]).astype(np.uint32)
    call_allele = np.array([x for c in calls for x in c], np.uint32)
    res = phase.phase_calls(eng, ev, region_hap_off, call_allele_off, call_allele, gt, n_samples, ploidy, fill=0xAB)
    a = dict(ev._asdict(), region_hap_off=region_hap_off)
    want = phase_cases.expected(phase_cases.unpack(a, call_allele_off, call_allele, gt), n_samples, ploidy, True, True)
    for k in phase.OUTPUTS:
        got, exp = getattr(res, k), want[k]
        assert got.dtype == exp.dtype and got.shape == exp.shape and np.array_equal(got, exp), (k, got.reshape(-1)[:16], exp.reshape(-1)[:16])
    assert res.call_rev_trim.tolist() == [100, 0, 0, 0, 0, 0, 0, 0] and res.call_end[0] == ev.vc_start[0]
    # the trimmed insertion (71 bytes) is found on its haplotype and phases with that haplotype's SNP; two plain alts or 65 map no
    # haplotype; the alts of 201 and 71 bytes are found on theirs; a difference in byte 69 alone is one
    assert res.phase_n_haps.tolist() == [1, 1, 0, 1, 0, 1, 1, 0] and res.phase_group.tolist() == [0, 0, -1, -1, -1, -1, -1, -1]
    assert np.flatnonzero(res.hap_in_call).tolist() == [0, 3, 9, 4 * 3 + 68, 4 * 3 + 68 + 1]
