"""phmm_trim_regions on the MI355X against the restatement of the reference's trimming stage (tests/region_trim_restatement.py),
through the C ABI as lorikeet_amd.trim binds it.  EQUALITY on every output array: it is all integers and bytes, there are no
tolerances.  The regions come from tests/region_trim_cases.py; tests/test_region_trim_oracle.py holds the restatement to the
reference's literals and to hand-derived expectations and counts on the CPU what the sets reach.  The module imports
lorikeet_amd.trim at the top: without the export every test here fails."""
import numpy as np
import pytest

import events_restatement as EV
import finalize_cases as FK
import finalize_restatement as FR
import region_trim_cases as K
import region_trim_restatement as R
from lorikeet_amd import _lib, events, finalize, trim
from lorikeet_amd.engine import HipPairHMMEngine, PhmmError

pytestmark = pytest.mark.gpu
SETS = K.sets()


@pytest.fixture(scope="module")
def eng():
    e = HipPairHMMEngine()
    yield e
    e.close()


def same(got, regions, dist, padding, tag):
    want = R.trim_batch(regions, dist, padding)
    for name, dt in trim.OUTPUTS:
        g, w = got[name], np.asarray(want[name], dt)
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist(), g[g != w][:8], w[g != w][:8])
    for name, rest in got["untouched"].items():      # behind the written part nothing is touched
        assert np.all(rest.view(np.uint8) == 0xAB), (tag, name)
    return want


def run(eng, s, regions=None, **kw):
    return trim.trim_regions(eng, s["regions"] if regions is None else regions, s["dist"], s["padding"], **kw)


@pytest.mark.parametrize("name", sorted(SETS))
def test_equals_the_restatement(eng, name):
    """each set in one call: the spans (0, 1, 63, 64, 65, 130 events, the extremes on lane 63 and lane 0, saturation, paddings
    cut on either side, deletions that only end or start inside, padding-only events, the repeat slice), the 200-element CIGAR
    and every status family beside healthy regions, order and duplicates at 1 .. 512 haplotypes, the 24 seeded regions with a
    region without haplotypes and one without variation"""
    s = SETS[name]
    want = same(run(eng, s, fill=0xAB), s["regions"], s["dist"], s["padding"], name)
    if name == "trim_edges":     # every family by name
        status = dict(zip(s["names"], want["region_status"]))
        for fam in ("LENGTH", "OPERATOR", "NOT_FOUND", "BUILDER", "REF_ELIMINATED"):
            assert status["status_" + fam] == getattr(trim, "STATUS_" + fam), fam
        assert status["status_LOCATION_left"] == status["status_LOCATION_right"] == trim.STATUS_LOCATION
        assert [status["event_" + f] for f in ("ALLELES", "BAD_OPERATOR", "BLOCK", "CIGAR_OVERRUN")] == [EV.ALLELES, EV.BAD_OPERATOR, EV.BLOCK, EV.CIGAR_OVERRUN]
        assert status["healthy_beside_them"] == 0 and status["first_panic_in_input_order_wins"] == trim.STATUS_LENGTH
    if name == "edge_spans":
        assert dict(zip(s["names"], want["region_status"]))["repeat_slice_underflow"] == trim.STATUS_REPEAT_SLICE


def test_every_small_cigar_against_every_span(eng):
    """every CIGAR of up to 4 elements over {M, I, D} with lengths 1 to 3 against every (start, stop): 134 065 haplotypes"""
    s = K.exhaustive_set()
    want = same(run(eng, s, fill=0xAB), s["regions"], s["dist"], s["padding"], "exhaustive")
    assert {trim.FATE_DUPLICATE, trim.FATE_CUT_IN_DELETION, trim.FATE_NOT_TRIMMED, 0, 1} <= set(want["hap_fate"])
    assert set(want["region_status"]) == {0, EV.BLOCK}     # (no trim panic: the spans lie inside the CIGARs)


@pytest.mark.parametrize("name", ["seeded", "order", "trim_edges"])
def test_a_region_alone_equals_the_same_region_in_a_batch_and_a_second_call(eng, name):
    s = SETS[name]
    first, again = run(eng, s), run(eng, s)
    for out, _ in trim.OUTPUTS:
        assert first[out].tobytes() == again[out].tobytes(), out
    ho = first["inputs"]["region_hap_off"]
    oo = first["out_region_hap_off"]
    for g in sorted({0, 5, 6, 11, len(s["regions"]) - 1}):
        alone = run(eng, s, [s["regions"][g]])
        for out, _ in trim.REGION_OUTPUTS + (("out_region_ref_hap", None),):
            assert first[out][g:g + 1].tobytes() == alone[out].tobytes(), (g, out)
        for out in ("hap_fate", "hap_dup_of"):
            assert first[out][ho[g]:ho[g + 1]].tobytes() == alone[out].tobytes(), (g, out)
        for out in ("out_hap_start_wrt_ref", "out_hap_source", "out_hap_is_ref"):
            assert first[out][oo[g]:oo[g + 1]].tobytes() == alone[out].tobytes(), (g, out)
        b0, b1 = first["out_hap_off"][oo[g]], first["out_hap_off"][oo[g + 1]]
        c0, c1 = first["out_hap_cigar_off"][oo[g]], first["out_hap_cigar_off"][oo[g + 1]]
        assert first["out_hap_bases"][b0:b1].tobytes() == alone["out_hap_bases"].tobytes(), g
        assert first["out_hap_cigar"][c0:c1].tobytes() == alone["out_hap_cigar"].tobytes(), g
        assert np.array_equal(first["out_hap_off"][oo[g]:oo[g + 1] + 1] - b0, alone["out_hap_off"]), g


def test_no_regions_and_regions_without_haplotypes(eng):
    o = trim.trim_regions(eng, [], fill=0xAB)
    assert o["n_out"] == 0 and list(o["out_region_hap_off"]) == [0] and list(o["out_hap_off"]) == [0] and list(o["out_hap_cigar_off"]) == [0]
    empty = [(b"ACGTACGT", 10, (12, 14), (10, 17), [])] * 3
    same(trim.trim_regions(eng, empty, fill=0xAB), empty, 0, K.DEFAULT, "no haplotypes")


def chain_regions(s, o):
    """what phmm_discover_events takes after the trim: the input's reference, the output's haplotypes, the new active span"""
    out = []
    for g, (ref, rs, _, _, _) in enumerate(s["regions"]):
        haps = []
        for k in range(o["out_region_hap_off"][g], o["out_region_hap_off"][g + 1]):
            bases = bytes(o["out_hap_bases"][o["out_hap_off"][k]:o["out_hap_off"][k + 1]])
            cigar = [int(c) for c in o["out_hap_cigar"][o["out_hap_cigar_off"][k]:o["out_hap_cigar_off"][k + 1]]]
            haps.append((bases, cigar, int(o["out_hap_start_wrt_ref"][k])))
        out.append(events.Region(ref, rs, haps, (int(o["new_active_start"][g]), int(o["new_active_end"][g])), 1 << 30))
    return out


def test_the_output_feeds_event_discovery_as_it_is(eng):
    """phmm_trim_regions -> phmm_discover_events on the output arrays with the new active span as window, equal to the two
    restatements chained"""
    s = SETS["seeded"]
    o = run(eng, s)
    keep = [g for g in range(len(s["regions"])) if o["variation_present"][g] and o["region_status"][g] == 0]
    got = events.discover_events(eng, [chain_regions(s, o)[g] for g in keep], s["dist"], with_haplotype_events=True)
    regions = []
    for g in keep:
        r = R.trim_region(s["regions"][g], s["dist"], s["padding"])
        regions.append(dict(ref=s["regions"][g][0], ref_start=s["regions"][g][1], haps=[(b, c, st) for b, c, st, _, _ in r["out"]],
                            window=r["new_active"], contig_length=1 << 30))
    want = EV.discover(regions, s["dist"])
    assert len(got.event_loc) > 20 and len(keep) >= 20
    for name in ("region_status", "region_event_off", "event_loc", "vc_start", "vc_end", "event_allele_off", "allele_length", "allele_kind",
                 "allele_bases_off", "allele_bases", "event_hap_allele", "hap_event_off", "hap_event_start", "hap_event_end", "hap_event_type"):
        g, w = getattr(got, name), want[name]
        w = np.frombuffer(bytes(w), np.uint8) if isinstance(w, (bytes, bytearray)) else np.asarray(w, g.dtype)
        assert np.array_equal(g, w), name


def test_the_new_padded_span_feeds_read_finalization_as_it_is(eng):
    """-> phmm_finalize_reads(PHMM_FIN_REGION) with the new padded span: reads laid across each region's padded span are
    hard-clipped to what the trimmer left, equal to the two restatements chained"""
    s = SETS["seeded"]
    o = run(eng, s)
    groups, want_groups = [], []
    for g, region in enumerate(s["regions"]):
        if not o["variation_present"][g] or o["region_status"][g]:
            continue
        r = R.trim_region(region, s["dist"], s["padding"])
        lo, hi = region[3]
        reads = [FK.read(c, pos=p) for p in range(max(lo - 30, 0), hi, 37) for c in ("60M", "10S40M5I10M", "20M4D30M")]
        groups.append(FK.group(reads, span=(int(o["new_padded_start"][g]), int(o["new_padded_end"][g]))))
        want_groups.append(FK.group(reads, span=r["new_padded"]))
    assert len(groups) >= 20
    res = finalize.finalize_reads(eng, groups, steps=_lib.PHMM_FIN_REGION)
    want = FR.finalize_reads(want_groups, steps=FR.FIN_REGION)
    assert len(want) == len(res.read_status) and len({int(k) for k in res.keep}) == 2
    for i, w in enumerate(want):
        for k in ("read_status", "keep", "new_pos", "clip_first", "clip_len"):
            assert int(getattr(res, k)[i]) == w[k], (i, k)
        assert [(int(x) & 15, int(x) >> 4) for x in res.cigar(i)] == w["out_cigar"], i


def broken(**change):
    a = trim.pack(K.seeded_set(4)["regions"])
    for k, v in change.items():
        a[k] = v(a[k].copy()) if callable(v) else v
    return a


def put(i, value):
    def f(x):
        x[i] = value
        return x
    return f


INVALID = {
    "padding NULL": (dict(), dict(omit=("padding",)), "padding"),
    "an output offset array NULL": (dict(), dict(omit=("out_hap_off",)), "output offsets"),
    "a region input NULL": (dict(), dict(omit=("region_active_end",)), "region inputs"),
    "a region output NULL": (dict(), dict(omit=("new_padded_end",)), "region outputs"),
    "a haplotype input NULL": (dict(), dict(omit=("hap_loc_start",)), "haplotype inputs"),
    "a haplotype output NULL": (dict(), dict(omit=("hap_fate",)), "haplotype outputs"),
    "the bases NULL": (dict(), dict(omit=("out_hap_bases",)), "bases, CIGARs"),
    "ref_bases NULL": (dict(), dict(omit=("ref_bases",)), "ref_bases"),
    "region_ref_off not from 0": (dict(region_ref_off=put(0, 1)), {}, "region_ref_off does not start at 0"),
    "region_hap_off not from 0": (dict(region_hap_off=put(0, 1)), {}, "region_hap_off does not start at 0"),
    "region_ref_off decreases": (dict(region_ref_off=put(2, 1)), {}, "region 1: region_ref_off not monotonic"),
    "region_hap_off decreases": (dict(region_hap_off=put(2, 1)), {}, "region 1: region_hap_off not monotonic"),
    "hap_off not from 0": (dict(hap_off=put(0, 1)), {}, "hap_off does not start at 0"),
    "hap_cigar_off not from 0": (dict(hap_cigar_off=put(0, 1)), {}, "hap_cigar_off does not start at 0"),
    "hap_off decreases": (dict(hap_off=put(3, 0)), {}, "haplotype 2: hap_off not monotonic"),
    "hap_cigar_off decreases": (dict(hap_cigar_off=put(3, 0)), {}, "haplotype 2: hap_cigar_off not monotonic"),
    "active span empty": (dict(region_active_end=put(1, 0)), {}, "region 1: the active span is not inside the padded span"),
    "active span outside the padded span": (dict(region_padded_start=put(2, 1 << 40)), {}, "region 2: the active span is not inside"),
    "a position beyond 2^62": (dict(region_padded_end=put(0, 1 << 62)), {}, "region 0: position beyond 2^62"),
    "a location that ends before it starts": (dict(hap_loc_end=put(4, 0), hap_loc_start=put(4, 9)), {}, "haplotype 4: its location ends before it starts"),
    "a haplotype position beyond 2^62": (dict(hap_loc_end=put(4, 1 << 62)), {}, "haplotype 4: position beyond 2^62"),
    "a start beyond 32 bits": (dict(hap_loc_end=put(4, 1 << 33)), {}, "haplotype 4: a trimmed start would not fit 32 bits"),
    "the 32-bit workspace index": (dict(hap_off=lambda x: np.concatenate([x[:-2], x[-2:] + np.uint32(1 << 31)])), {},
                                   "haplotype bases + CIGAR elements + 8 per haplotype reach 2^31"),
    "a reference base outside the alphabet": (dict(ref_bases=put(7, ord("*"))), {}, "reference base 7"),
    "a haplotype base outside the alphabet": (dict(hap_bases=put(9, ord("."))), {}, "haplotype base 9"),
    "an unknown operator": (dict(hap_cigar=put(1, (3 << 4) | 9)), {}, "CIGAR element 1"),
    "an element of length 0": (dict(hap_cigar=put(1, 0)), {}, "CIGAR element 1"),
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_arguments_are_refused_by_name_and_nothing_is_written(eng, name):
    change, kw, message = INVALID[name]
    with pytest.raises(PhmmError) as e:
        trim.trim_regions(eng, broken(**change), 1, K.SMALL, fill=0xAB, **kw)
    assert e.value.code == _lib.PHMM_ERR_INVALID_ARG and message in str(e.value), str(e.value)
    for k, v in e.value.outputs.items():
        assert np.all(v.view(np.uint8) == 0xAB), k


def test_the_limits_are_refused_by_name(eng):
    ref = b"A" * (_lib.PHMM_EVENTS_MAX_REF + 1)
    with pytest.raises(PhmmError) as e:
        trim.trim_regions(eng, [(ref, 0, (1, 2), (0, 3), [])])
    assert "region 0: 16385 reference bases, more than 16384" in str(e.value)
    hap = (b"ACGT", "4M", 0, (0, 3), False)
    with pytest.raises(PhmmError) as e:
        trim.trim_regions(eng, [(b"ACGT", 0, (1, 2), (0, 3), [hap] * (_lib.PHMM_EVENTS_MAX_HAPS + 1))])
    assert "region 0: 513 haplotypes, more than 512" in str(e.value)


def test_the_largest_region_is_taken(eng):
    """512 haplotypes over 16 384 reference bases: the limits themselves"""
    import random
    rng = random.Random(16)
    ref = K.rand_ref(rng, _lib.PHMM_EVENTS_MAX_REF)
    haps = [K.make_hap(ref, 0, (), True)] + [K.make_hap(ref, 0, K.snps(ref, sorted(rng.sample(range(200, 16000), 3)))) for _ in range(511)]
    region = [(ref, 0, (100, 16300), (0, 16383), haps)]
    same(trim.trim_regions(eng, region, 0, K.DEFAULT, fill=0xAB), region, 0, K.DEFAULT, "largest")
