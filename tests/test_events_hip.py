"""phmm_discover_events on the MI355X against the restatement of the head of the reference's assign_genotype_likelihoods
(tests/events_restatement.py): through the C ABI, EQUALITY on every output array -- integer and byte work has no tolerance.
The regions come from tests/events_cases.py; tests/test_events_oracle.py checks on the CPU what they exercise.  The module
imports lorikeet_amd.events at the top: without the call every test here fails."""
import numpy as np
import pytest

import events_cases as K
import events_restatement as R
from lorikeet_amd import _lib, events, genotype
from lorikeet_amd.engine import HipPairHMMEngine, PhmmError

pytestmark = pytest.mark.gpu
DENSE = ("region_event_off", "region_status", "event_region", "event_allele_off", "event_start", "event_end", "event_loc", "vc_start",
         "vc_end", "event_flags", "event_hap_allele", "allele_length", "allele_kind", "allele_bases_off")
HAPS = ("hap_event_off", "hap_event_start", "hap_event_end", "hap_event_ref_length", "hap_event_alt_off", "hap_event_type")


@pytest.fixture(scope="module")
def eng():
    e = HipPairHMMEngine()
    yield e
    e.close()


def run(eng, regions, dist=0, include_spanning=True, margin=2, maps=True, **kw):
    return events.discover_events(eng, regions, dist, include_spanning, margin, with_haplotype_events=maps, **kw)


def same(res, want, tag, maps=True):
    for k in DENSE + (HAPS if maps else ()):
        assert np.asarray(getattr(res, k)).tolist() == list(want[k]), (tag, k, np.asarray(getattr(res, k)).tolist(), want[k])
    assert bytes(res.allele_bases) == bytes(want["allele_bases"]), (tag, bytes(res.allele_bases), want["allele_bases"])
    if maps:
        assert bytes(res.hap_event_alt) == bytes(want["hap_event_alt"]), (tag, bytes(res.hap_event_alt), want["hap_event_alt"])
    n = [len(want["event_region"]), len(want["allele_length"]), len(want["allele_bases"]), len(want["event_hap_allele"])]
    n += [len(want["hap_event_start"]), len(want["hap_event_alt"])] if maps else [0, 0]
    assert res.required.tolist() == n, (tag, res.required.tolist(), n)


def check(eng, regions, tag, dist=0, include_spanning=True, margin=2):
    res = run(eng, regions, dist, include_spanning, margin)
    same(res, R.discover(regions, dist, include_spanning, margin), tag)
    return res


def test_hand_built_single_haplotypes(eng):
    """Every adjacent operator pair, indels at the ends and at ref_pos 0, the blocks, the statuses, bases that are not regular,
    M blocks around 64 bases: one region per call, and all of them in one call per distance."""
    cases = K.singles()
    for name, rg, dists in cases:
        for d in dists:
            check(eng, [rg], (name, d), d)
    for d in (0, 1, 3):
        check(eng, [rg for _, rg, _ in cases], ("all", d), d)


def test_several_haplotypes(eng):
    for name, rg, o in K.multis():
        check(eng, [rg], name, o.get("dist", 0), o.get("include_spanning", True), o.get("margin", 2))
    for spanning in (True, False):
        check(eng, [rg for _, rg, _ in K.multis()], ("all", spanning), 0, spanning, 3)


def golden_regions():
    """The reference's own cases as regions: tests/golden/event_map_cases.json (see its extraction script)."""
    g = K.golden()
    out = []
    for row in g["test_mnps"]:
        rg = K.region(row["ref"].encode(), [(row["hap"].encode(), R.parse_cigar(row["cigar"]), 0)], ref_start=1, window=(1, len(row["ref"])))
        for d in row["distances"]:
            out.append(("mnps", rg, d, row["expected"]))
    for row in g["test_get_overlapping_events"]:
        rg = K.region(g["overlapping_ref"].encode(), [(row["hap"].encode(), R.parse_cigar(row["cigar"]), g["overlapping_hap_start"])], ref_start=1,
                      window=(row["loc"], row["loc"]))
        out.append(("overlapping", rg, 1, row))
    return out


def test_reference_cases(eng):
    """test_mnps (every row, each distance) and test_get_overlapping_events through the device, against the expectations the
    reference's tests state -- not only against the restatement; with the per-haplotype outputs."""
    for kind, rg, d, exp in golden_regions():
        res = check(eng, [rg], (kind, exp), d)
        alts = [bytes(res.hap_event_alt[a:b]).decode() for a, b in zip(res.hap_event_alt_off[:-1], res.hap_event_alt_off[1:])]
        refs = [rg["ref"][s - 1:s - 1 + n].decode() for s, n in zip(res.hap_event_start.tolist(), res.hap_event_ref_length.tolist())]
        if kind == "mnps":
            assert [[r, a] for r, a in zip(refs, alts)] == exp, (exp, refs, alts)
        else:  # the locus is the whole window: the events overlapping it that start there, or a '*' for one that spans it
            loc = exp["loc"]
            over = [(r, a) for r, a, s, e in zip(refs, alts, res.hap_event_start.tolist(), res.hap_event_end.tolist()) if s <= loc <= e]
            if exp["ref"] is None:
                assert not over, (exp, over)
            else:
                assert (exp["ref"], exp["alt"]) in over, (exp, over)


def test_reference_block_cases(eng):
    """test_make_blocks: each row as a CIGAR that proposes the two events at one start.  A deletion can only be proposed
    before an insertion of the same start by a zero-length element, so the two deletion-first rows run insertion first --
    the block is the same (the CPU test holds make_block to the rows as they stand)."""
    for first, second, expected in K.golden()["test_make_blocks"]:
        ref = b"CCCC" + (first[0] if len(first[0]) > len(second[0]) else second[0]).encode() + b"TTTT"
        if len(first[0]) == len(first[1]):  # SNP, then an indel
            hap, cig = bytearray(ref[:4] + first[1].encode()), [(0, 5)]
            rest = [second]
        else:
            hap, cig = bytearray(ref[:5]), [(0, 5)]
            rest = sorted([first, second], key=lambda a: len(a[0]))  # insertion, then deletion
        pos = 5
        for r, a in rest:
            if len(a) > len(r):
                hap += a[1:].encode()
                cig.append((1, len(a) - 1))
            else:
                cig.append((2, len(r) - 1))
                pos += len(r) - 1
        hap += ref[pos:]
        cig.append((0, len(ref) - pos))
        res = check(eng, [K.region(ref, [(bytes(hap), cig, 0)], ref_start=16)], (first, second))
        assert res.hap_event_start.tolist() == [20] and res.hap_event_ref_length.tolist() == [len(expected[0])]
        assert bytes(res.hap_event_alt).decode() == expected[1], (first, second, bytes(res.hap_event_alt))


def test_reference_allele_mapper_cases(eng):
    """get_event_mapper_data and get_variant_contexts_from_active_haplotypes_data: their event maps rebuilt as haplotypes over
    one reference (positions and allele lengths as recorded; the bases are the reference's own, because the recorded alleles
    of different test haplotypes contradict each other), the expected events by (start, end).  The reference's test asks
    get_variant_contexts_from_active_haplotypes at a locus of its choice; the call only visits loci where an event starts, so
    where none of the recorded events starts at the locus one more haplotype, the last, carries a SNP there: its event then is
    the last of the expected ones.  Against the recorded expectations this test holds the device to the number of events, the
    number of alleles and vc_end only: with other bases the recorded alleles cannot be compared.  The recorded alleles and the
    expected haplotype -> allele map are held to the restatement on the CPU (tests/test_events_oracle.py) and reach the device
    through its equality with the restatement on every array."""
    for case in K.golden()["active_haplotypes"]:
        case = dict(case)
        if case["expected"] and not any(v["start"] == case["loc"] for v in case["expected"]):
            helper = dict(start=case["loc"], end=case["loc"], ref="A", alt="C", type="Snp")
            case["haplotypes"] = case["haplotypes"] + [[helper]]
            case["expected"] = case["expected"] + [helper]
        lo = min([case["loc"]] + [v["start"] for h in case["haplotypes"] for v in h]) - 3
        hi = max([case["loc"]] + [v["end"] for h in case["haplotypes"] for v in h]) + 4
        rng = np.random.default_rng(5)
        ref = bytes(rng.choice(list(b"ACGT"), hi - lo).astype(np.uint8))
        haps = []
        for h in case["haplotypes"]:
            script, pos = [], 0
            for v in sorted(h, key=lambda v: v["start"]):
                at = v["start"] - lo
                if len(v["ref"]) == len(v["alt"]):
                    script += [("M", at - pos), ("M", 1, 0)]
                    pos = at + 1
                elif len(v["ref"]) > len(v["alt"]):
                    script += [("M", at + 1 - pos), ("D", len(v["ref"]) - 1)]
                    pos = at + len(v["ref"])
                else:
                    script += [("M", at + 1 - pos), ("I", b"T" * (len(v["alt"]) - 1))]
                    pos = at + 1
            script.append(("M", hi - lo - pos))
            haps.append(K.build(ref, [s for s in script if s[1]], 0))
        rg = K.region(ref, haps, ref_start=lo, window=(case["loc"], case["loc"]), contig_length=20000000)
        res = check(eng, [rg], case["name"])
        want = case["expected"]
        assert len(res.event_loc) == (1 if want else 0), (case["name"], res.event_loc)
        if want:  # the merged context: one alt per expected event ('*' once for all that span), the longest span
            starts_here = [v for v in want if v["start"] == case["loc"]]
            n_alt = len(starts_here) + (len(starts_here) < len(want))
            assert int(res.event_allele_off[1]) == 1 + n_alt, (case["name"], res.event_allele_off, want)
            assert int(res.vc_end[0]) == max([case["loc"]] + [v["end"] for v in starts_here])


def test_seeded_random_regions_and_properties(eng):
    """Random haplotypes made from the reference by edits; a region alone equals the region inside a batch, permuting regions
    permutes the output, two runs are byte-identical."""
    for name, regions, d in K.random_batches():
        res = check(eng, regions, name, d)
        again = run(eng, regions, d)
        for a, b in zip(res, again):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), name
        if len(regions) > 1:
            pick = sorted({0, 1, len(regions) // 2, len(regions) - 1})
            for g in pick:  # alone
                same(run(eng, [regions[g]], d), R.discover([regions[g]], d), (name, "alone", g))
                a, b = int(res.region_event_off[g]), int(res.region_event_off[g + 1])
                alone = run(eng, [regions[g]], d)
                assert alone.event_loc.tolist() == res.event_loc[a:b].tolist()
                assert bytes(alone.allele_bases) == bytes(res.allele_bases[int(res.allele_bases_off[res.event_allele_off[a]]):int(res.allele_bases_off[res.event_allele_off[b]])])
            perm = np.random.default_rng(3).permutation(len(regions)).tolist()
            shuffled = [regions[i] for i in perm]
            same(run(eng, shuffled, d), R.discover(shuffled, d), (name, "permuted"))


def test_capacity(eng):
    """Each of the four capacities (and the two of the optional outputs), one too small: the new error, the exact sizes,
    sentinel-filled outputs untouched; the reported sizes then succeed; a larger call on the same engine stays equal."""
    regions = [rg for _, rg, _ in K.multis()]
    want = R.discover(regions)
    need = run(eng, regions).required.tolist()
    assert all(need), need
    for k in range(6):
        cap = list(need)
        cap[k] -= 1
        with pytest.raises(PhmmError) as err:
            run(eng, regions, capacity=cap, fill=0xA5)
        assert err.value.code == _lib.PHMM_ERR_EVENT_CAPACITY and err.value.required.tolist() == need, (k, err.value.required)
        for name, arr in err.value.outputs.items():
            if name != "required":
                assert np.all(arr.view(np.uint8) == 0xA5), (k, name)
    same(run(eng, regions, capacity=need, fill=0xA5), want, "exact")
    roomy = run(eng, regions, capacity=[n + 7 for n in need], fill=0xA5)
    same(roomy, want, "roomy")
    big = [rg for _, b, _ in K.random_batches() for rg in b] * 3  # grows the staging buffer
    same(run(eng, big, 1), R.discover(big, 1), "larger call")
    same(run(eng, regions), want, "small again")
    without = run(eng, regions, maps=False)
    same(without, want, "no maps", maps=False)
    assert without.hap_event_off is None


def test_chain_into_the_per_event_calls(eng):
    """The arrays as they are, with seeded likelihoods, through phmm_genotype_likelihoods -> phmm_allele_frequency ->
    phmm_assign_genotypes -> phmm_annotate_events: accepted, and equal to what the restatement's arrays give."""
    rng = np.random.default_rng(11)
    regions = [K.random_region(rng, 80, 5), K.random_region(rng, 120, 8), K.region(K.REF40, [])]
    res, want = run(eng, regions, maps=False), R.discover(regions)
    n_reads = [6, 9, 0]
    nh = [len(r["haps"]) for r in regions]
    read_off = np.concatenate([[0], np.cumsum(n_reads)]).astype(np.uint32)
    hap_off = np.concatenate([[0], np.cumsum(nh)]).astype(np.uint32)
    out_off = np.concatenate([[0], np.cumsum([a * b for a, b in zip(n_reads, nh)])]).astype(np.uint64)
    lk = -rng.random(int(out_off[-1])) * 8
    sample = rng.integers(0, 2, int(read_off[-1])).astype(np.uint32)
    starts = np.concatenate([np.full(n, r["ref_start"], np.int64) for n, r in zip(n_reads, regions)])
    ends = np.concatenate([np.full(n, r["ref_start"] + len(r["ref"]) - 1, np.int64) for n, r in zip(n_reads, regions)])

    # the per-event wrappers take these very arrays: call the C ABI through them
    lib, C = eng.lib, __import__("ctypes")
    p = lambda x, t: x.ctypes.data_as(t)  # noqa: E731
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    def gls(a):
        er, ao = np.ascontiguousarray(a["event_region"], np.uint32), np.ascontiguousarray(a["event_allele_off"], np.uint32)
        es, ee = np.ascontiguousarray(a["event_start"], np.int64), np.ascontiguousarray(a["event_end"], np.int64)
        hm = np.ascontiguousarray(list(a["event_hap_allele"]) + [0], np.int32)
        n_ev = len(er)
        G = [genotype.genotype_count(2, int(ao[e + 1] - ao[e])) for e in range(n_ev)]
        gl_off = np.concatenate([[0], np.cumsum([2 * g for g in G])]).astype(np.uint64)
        gl, pl = np.zeros(int(gl_off[-1])), np.zeros(int(gl_off[-1]), np.int32)
        code = lib.phmm_genotype_likelihoods(eng._h, 3, p(read_off, _lib.u32p), p(hap_off, _lib.u32p), p(out_off, _lib.u64p), p(lk, _lib.f64p),
                                             None, p(sample, _lib.u32p), p(starts, i64p), p(ends, i64p), 2, 2, n_ev, p(er, _lib.u32p),
                                             p(ao, _lib.u32p), p(es, i64p), p(ee, i64p), p(hm, i32p), p(gl_off, _lib.u64p),
                                             p(gl, _lib.f64p), p(pl, i32p), None)
        assert code == _lib.PHMM_OK, eng.last_error()
        ln, kd = np.ascontiguousarray(a["allele_length"], np.uint32), np.ascontiguousarray(a["allele_kind"], np.uint8)
        af = genotype.allele_frequency(eng, pl, gl_off, ao, ln, kd, n_samples=2, ploidy=2)
        asg = genotype.assign_genotypes(eng, af, pl, ao, gl_off, ln, kd, n_samples=2, ploidy=2)
        call = genotype.call_alleles_of(af)
        c_off = np.concatenate([[0], np.cumsum([len(c) for c in call])]).astype(np.uint32)
        ca = np.array([x for c in call for x in c] + [0], np.uint32)
        n_c = int(c_off[-1])
        ad, afr = np.zeros(2 * n_c + 1, np.int32), np.zeros(2 * n_c + 1)
        dp, ac = np.zeros(2 * n_ev + 1, np.int32), np.zeros(2 * n_ev + 1, np.uint32)
        mq, info_dp, qd_depth, qd, fl = np.zeros(n_c + 1, np.uint8), np.zeros(n_ev + 1, np.int32), np.zeros(n_ev + 1, np.int32), np.zeros(n_ev + 1), np.zeros(n_ev + 1, np.uint32)
        mapq = np.full(int(read_off[-1]), 60, np.uint8)
        lpe = np.ascontiguousarray(np.asarray(af.qual, np.float64) / -10.0)
        code = lib.phmm_annotate_events(eng._h, 3, p(read_off, _lib.u32p), p(hap_off, _lib.u32p), p(out_off, _lib.u64p), p(lk, _lib.f64p), None,
                                        p(sample, _lib.u32p), p(starts, i64p), p(ends, i64p), p(mapq, _lib.u8p), 2, n_ev, p(er, _lib.u32p),
                                        p(ao, _lib.u32p), p(es, i64p), p(ee, i64p), p(hm, i32p), p(c_off, _lib.u32p), p(ca, _lib.u32p),
                                        None, None, None, None, None, None, None, None, p(lpe, _lib.f64p), None, p(ad, i32p), p(dp, i32p),
                                        p(afr, _lib.f64p), p(ac, _lib.u32p), p(mq, _lib.u8p), None, p(info_dp, i32p), p(qd_depth, i32p),
                                        p(qd, _lib.f64p), p(fl, _lib.u32p))
        assert code == _lib.PHMM_OK, eng.last_error()
        return [gl.tobytes(), pl.tobytes(), np.asarray(af.qual).tobytes(), asg.gt.tobytes(), asg.gq.tobytes(), ad.tobytes(), dp.tobytes(),
                afr.tobytes(), mq.tobytes(), qd.tobytes()]

    got = gls({k: getattr(res, k) for k in DENSE if k.startswith("event") or k.startswith("allele")})
    assert len(res.event_region) > 10
    assert got == gls(want)


def test_invalid_arguments(eng):
    """Each PHMM_ERR_INVALID_ARG condition of the header: the code, the offender in phmm_last_error, nothing written."""
    ok = K.region(K.REF40, [K.build(K.REF40, [("M", 20, 4)], 2)])
    a = events.pack([ok])

    def bad(tag, **change):
        b = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in a.items()}
        b.update(change)
        with pytest.raises(PhmmError) as err:
            events.discover_events(eng, b, with_haplotype_events=True, capacity=[64] * 6, fill=0x5A, omit=b.pop("omit", ()))
        assert err.value.code == _lib.PHMM_ERR_INVALID_ARG, tag
        for name, arr in err.value.outputs.items():
            assert np.all(arr.view(np.uint8) == 0x5A), (tag, name)
        return str(err.value)

    u32 = lambda *x: np.array(x, np.uint32)  # noqa: E731
    u64 = lambda *x: np.array(x, np.uint64)  # noqa: E731
    assert "region_ref_off" in bad("ref offsets", region_ref_off=u32(40, 0))
    assert "region_hap_off" in bad("hap offsets", region_hap_off=u32(1, 0))
    assert "hap_off" in bad("hap_off", hap_off=u32(20, 0))
    assert "hap_cigar_off" in bad("cigar offsets", hap_cigar_off=u32(1, 0))
    assert "contig" in bad("contig length", region_contig_length=u64(0))
    assert "2^62" in bad("position", region_ref_start=u64(1 << 62))
    base = a["ref_bases"].copy()
    base[7] = ord("*")
    assert "reference base 7" in bad("reference base", ref_bases=base)
    base = a["hap_bases"].copy()
    base[3] = ord("<")
    assert "haplotype base 3" in bad("haplotype base", hap_bases=base)
    assert "CIGAR element 0" in bad("operator", hap_cigar=u32((20 << 4) | 9))
    assert "CIGAR element 0" in bad("zero length", hap_cigar=u32(0))
    # offsets start at 0
    assert "region_ref_off does not start at 0" in bad("ref offsets from 1", region_ref_off=u32(1, 40))
    assert "region_hap_off does not start at 0" in bad("hap offsets from 1", region_hap_off=u32(1, 1))
    assert "hap_off does not start at 0" in bad("hap_off from 1", hap_off=u32(1, 20))
    assert "hap_cigar_off does not start at 0" in bad("cigar offsets from 1", hap_cigar_off=u32(1, 1))
    # 2^31 haplotype bases and CIGAR elements: the host refuses before it reads a base or an element
    assert "2^31" in bad("work, bases", hap_off=u32(0, 0x80000000))
    assert "2^31" in bad("work, elements", hap_cigar_off=u32(0, 0x80000000))
    assert "2^31" in bad("work, together", hap_off=u32(0, 0x7FFFFFF0), hap_cigar_off=u32(0, 8))
    # the seven per-haplotype map outputs come together: hap_event_off without one of the other six
    for name in ("hap_event_start", "hap_event_end", "hap_event_ref_length", "hap_event_alt_off", "hap_event_alt", "hap_event_type"):
        assert "come together" in bad(name, omit=(name,))
    # a required output, one at a time
    for name in ("required", "region_event_off", "region_status", "event_region", "event_allele_off", "event_start", "event_end", "event_loc",
                 "vc_start", "vc_end", "event_flags", "event_hap_allele", "allele_length", "allele_kind", "allele_bases_off", "allele_bases"):
        assert "null array" in bad(name, omit=(name,))
    long_ref = K.region(b"A" * (_lib.PHMM_EVENTS_MAX_REF + 1), [])
    many = K.region(K.REF40, [(b"ACGT", [(0, 4)], 0)] * (_lib.PHMM_EVENTS_MAX_HAPS + 1))
    for tag, rg in (("reference bases", long_ref), ("haplotypes", many)):
        with pytest.raises(PhmmError) as err:
            run(eng, [rg])
        assert err.value.code == _lib.PHMM_ERR_INVALID_ARG and tag in str(err.value)
    null = eng.lib.phmm_discover_events(eng._h, 1, *([None] * 12), 0, 1, 2, *([None] * 24))
    assert null == _lib.PHMM_ERR_INVALID_ARG and "null" in eng.last_error()
    # the limits themselves are fine, and so are no regions and regions without haplotypes
    at_limit = K.region(b"ACGT" * (_lib.PHMM_EVENTS_MAX_REF // 4), [(b"ACGA", [(0, 4)], _lib.PHMM_EVENTS_MAX_REF - 4)] * _lib.PHMM_EVENTS_MAX_HAPS)
    check(eng, [at_limit], "at the limits")
    check(eng, [], "no regions")
    check(eng, [K.region(K.REF40, []), K.region(K.REF40, [])], "no haplotypes")
