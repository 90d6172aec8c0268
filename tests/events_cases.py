"""Test infrastructure: the regions tests/test_events_hip.py sends through phmm_discover_events, and what
tests/test_events_oracle.py counts in them on the CPU.  A region is a dict(ref, ref_start, haps [(bases, cigar [(op, len)],
hap_start)], window, contig_length), what events_restatement.discover takes."""
import json
import os

import numpy as np

import events_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "event_map_cases.json")
REF40 = b"ACGTTGCAAGCTTAGGCATCGATTGACCTGAAGTCCTAGA"
FLIP = {65: 67, 67: 71, 71: 84, 84: 65}  # A -> C -> G -> T -> A


def region(ref, haps, ref_start=100, window=None, contig_length=1000000):
    return dict(ref=bytes(ref), ref_start=ref_start, haps=[(bytes(b), list(c), s) for b, c, s in haps],
                window=window or (ref_start, ref_start + len(ref) - 1), contig_length=contig_length)


def build(ref, script, start=0):
    """A haplotype from the reference by an edit script, so that CIGAR and bases agree: ("M", n, mismatch offsets...),
    ("I", bases), ("D", n), ("S", bases), ("N" / "H" / "P", n).  Returns (bases, cigar, start)."""
    pos, hap, cig = start, bytearray(), []
    for op in script:
        k = op[0]
        if k in "M=X":
            seg = bytearray(ref[pos:pos + op[1]])
            for o in op[2:]:
                seg[o] = FLIP.get(seg[o], seg[o])
            hap += seg
            pos += op[1]
            cig.append((R.OPS.index(k), op[1]))
        elif k in "IS":
            hap += op[1]
            cig.append((R.OPS.index(k), len(op[1])))
        else:
            pos += op[1] if k in "DN" else 0
            cig.append((R.OPS.index(k), op[1]))
    return bytes(hap), cig, start


def singles():
    """Hand-built single haplotypes: (name, region, distances)."""
    out = []

    def add(name, script, ref=REF40, start=0, dists=(0,), **kw):
        out.append((name, region(ref, [build(ref, script, start)], **kw), dists))

    el = {"M": [("M", 3, 2), ("M", 3, 0)], "I": [("I", b"GT"), ("I", b"C")], "D": [("D", 2), ("D", 3)], "S": [("S", b"TT"), ("S", b"A")]}
    for a in "MIDS":  # every adjacent operator pair, inside the alignment ("II" fails in make_block: status)
        for b in "MIDS":
            add("pair_%s%s" % (a, b), [("M", 5), el[a][0], el[b][1], ("M", 5)], start=2, dists=(0, 1))
    add("ins_first", [("I", b"GG"), ("M", 10, 3)], start=3)
    add("ins_last", [("M", 10, 3), ("I", b"GG")], start=3)
    add("del_first", [("D", 2), ("M", 10, 3)], start=3)
    add("del_last", [("M", 10, 3), ("D", 2)], start=3)
    add("ins_at_ref_pos_0", [("S", b"AA"), ("I", b"GG"), ("M", 10, 3)])
    add("del_at_ref_pos_0", [("S", b"AA"), ("D", 2), ("M", 10, 3)])
    add("snp_then_ins", [("M", 6, 5), ("I", b"TT"), ("M", 6)], start=1)
    add("snp_then_del", [("M", 6, 5), ("D", 3), ("M", 6)], start=1)
    add("snp_then_ins_del", [("M", 6, 5), ("I", b"TT"), ("D", 3), ("M", 6)], start=1)
    add("snp_ins_ins", [("M", 6, 5), ("I", b"TT"), ("I", b"G"), ("M", 6)], start=1)
    add("ins_then_del", [("M", 6), ("I", b"TT"), ("D", 3), ("M", 6)], start=1)
    add("del_then_ins", [("M", 6), ("D", 3), ("I", b"TT"), ("M", 6)], start=1)
    add("5D_2I_3D", [("M", 6), ("D", 5), ("I", b"TT"), ("D", 3), ("M", 6)], start=1)
    add("ins_del_ins", [("M", 6), ("I", b"TT"), ("D", 3), ("I", b"G"), ("M", 6)], start=1)
    add("two_insertions", [("M", 6), ("I", b"TT"), ("I", b"G"), ("M", 6)], start=1)
    for k in "NPH":
        add("operator_" + k, [("M", 6, 2), (k, 2), ("M", 6)], start=1)
    add("operator_N_after_two_insertions", [("M", 6), ("I", b"TT"), ("I", b"G"), ("N", 2), ("M", 6)], start=1)
    add("eq_and_x", [("=", 6), ("X", 3, 0, 1, 2), ("=", 6)], start=1, dists=(0, 1))
    add("overrun_reference", [("M", 6), ("D", 40), ("M", 2)], start=1)
    add("overrun_reference_M", [("M", 38)], ref=REF40 + b"AC", start=5, window=(100, 160))
    out.append(("overrun_haplotype", region(REF40, [(b"ACGTT", [(0, 8)], 0)]), (0,)))
    out.append(("overrun_haplotype_ins", region(REF40, [(b"ACGTT", [(0, 4), (1, 3), (0, 2)], 0)]), (0,)))
    out.append(("start_past_reference", region(REF40, [(b"ACGTT", [(1, 1), (1, 2), (0, 2)], 50)]), (0,)))
    out.append(("del_at_0_past_reference", region(REF40, [(b"ACGTT", [(2, 60), (4, 5)], 0)]), (0,)))
    # bases that are not regular (N), and lower case, which is ("ACGTacgt")
    n_ref = bytearray(REF40)
    n_ref[12] = ord("N")
    add("N_in_reference_mismatch", [("M", 20, 3)], ref=bytes(n_ref), start=5)  # offset 7 is the N: no event there
    out.append(("N_in_reference_under_snp", region(bytes(n_ref), [(REF40[5:25], [(0, 20)], 5)]), (0, 1)))
    add("N_inside_deletion", [("M", 6), ("D", 4), ("M", 6)], ref=bytes(n_ref), start=4)
    add("N_as_deletion_anchor", [("M", 8), ("D", 2), ("M", 6)], ref=bytes(n_ref), start=5)
    add("N_as_insertion_anchor", [("M", 8), ("I", b"GG"), ("M", 6)], ref=bytes(n_ref), start=5)
    add("N_inside_insertion", [("M", 6), ("I", b"GNG"), ("M", 6)], start=4)
    add("n_inside_insertion", [("M", 6), ("I", b"GnG"), ("M", 6)], start=4)
    add("lower_case_insertion", [("M", 6), ("I", b"gat"), ("M", 6)], start=4)
    hap = bytearray(REF40[4:20])
    hap[3] = ord("N")
    hap[8] = ord("t") if REF40[12:13] != b"T" else ord("c")
    out.append(("N_and_lower_case_in_haplotype", region(REF40, [(bytes(hap), [(0, 16)], 4)]), (0, 1, 3)))
    low = bytearray(REF40)
    low[10] = ord(bytes(low[10:11]).lower())
    out.append(("lower_case_reference_same_base", region(bytes(low), [(REF40[4:20], [(0, 16)], 4)]), (0,)))  # 'g' against 'G'
    add("lower_case_reference_other_base", [("M", 16, 6)], ref=bytes(low), start=4, dists=(0, 1))
    add("lower_case_reference_in_deletion", [("M", 5), ("D", 3), ("M", 6)], ref=bytes(low), start=4)
    out.append(("lower_case_snp_then_ins", region(bytes(low), [(REF40[4:11] + b"TT" + REF40[11:17], [(0, 7), (1, 2), (0, 6)], 4)]), (0,)))
    # M blocks around the width of a wave
    rng = np.random.default_rng(7)
    ref = bytes(rng.choice(list(b"ACGT"), 140).astype(np.uint8))
    for n in (63, 64, 65, 129):
        offs = sorted({o for o in (0, 63, 64, n - 1) if o < n})
        add("M%d" % n, [("M", 3), ("I", b"G"), ("M", n) + tuple(offs), ("D", 2), ("M", 3)], ref=ref, start=1, dists=(0, 1, 3), window=(100, 300))
        add("M%d_dense" % n, [("M", n) + tuple(range(0, n, 2))], ref=ref, start=2, dists=(0, 1, 3), window=(100, 300))
    return out


def multis():
    """Several haplotypes: (name, region, dict of options)."""
    out = []
    homo = b"CCGTAAAAAGTCCATG"
    h = lambda script, start=0, ref=REF40: build(ref, script, start)  # noqa: E731
    out.append(("homopolymer", region(homo, [h([("M", 4), ("D", 1), ("M", 11)], 0, homo), h([("M", 4), ("D", 2), ("M", 10)], 0, homo),
                                           h([("M", 16)], 0, homo)]), {}))
    span = [h([("M", 10), ("D", 6), ("M", 10)], 2), h([("M", 30, 12)], 2), h([("M", 30)], 2)]
    out.append(("deletion_spans_snp", region(REF40, span), {}))
    out.append(("deletion_spans_snp_spanning_off", region(REF40, span), dict(include_spanning=False)))
    out.append(("two_spanning_deletions", region(REF40, [h([("M", 10), ("D", 6), ("M", 10)], 2), h([("M", 9), ("D", 8), ("M", 10)], 2),
                                                        h([("M", 30, 13)], 2), h([("M", 30)], 2)]), {}))
    out.append(("deletion_ends_where_insertion_starts", region(REF40, [h([("M", 8), ("D", 4), ("M", 12)], 2), h([("M", 12), ("I", b"GG"), ("M", 12)], 2),
                                                                      h([("M", 8), ("D", 4), ("I", b"GG"), ("M", 12)], 2)]), {}))
    out.append(("mnp_ends_where_insertion_starts", region(REF40, [h([("M", 12, 9, 11), ("I", b"GG"), ("M", 12)], 2), h([("M", 12), ("I", b"GG"), ("M", 12)], 2)]),
                dict(dist=2)))
    out.append(("5D_2I_3D_beside_others", region(REF40, [h([("M", 6), ("D", 5), ("I", b"TT"), ("D", 3), ("M", 6)], 1), h([("M", 30, 11)], 1),
                                                        h([("M", 11), ("I", b"TT"), ("M", 10)], 1)]), {}))
    same = h([("M", 10, 4), ("I", b"AC"), ("M", 10)], 3)
    out.append(("same_event_on_several", region(REF40, [same, h([("M", 20)], 3), same, same]), {}))
    out.append(("event_on_later_haplotype_only", region(REF40, [h([("M", 20)], 3), h([("M", 20)], 3), h([("M", 20, 7)], 3)]), {}))
    out.append(("block_equals_shorter_deletion", region(b"TTAGGGGGCATCGATT", [h([("M", 3), ("I", b"GGG"), ("D", 4), ("M", 9)], 0, b"TTAGGGGGCATCGATT"),
                                                                             h([("M", 3), ("D", 1), ("M", 12)], 0, b"TTAGGGGGCATCGATT")]), {}))
    out.append(("alt_equals_reference", region(b"TTAGGGGGCATCGATT", [h([("M", 3), ("D", 1), ("M", 12)], 0, b"TTAGGGGGCATCGATT"),
                                                                    h([("M", 3), ("I", b"GG"), ("D", 3), ("M", 10)], 0, b"TTAGGGGGCATCGATT")]), {}))
    out.append(("merge_loses_reference", region(b"TTAGGGGGCATCGATT", [h([("M", 3), ("I", b"GG"), ("D", 2), ("M", 11)], 0, b"TTAGGGGGCATCGATT"),
                                                                     h([("M", 3), ("D", 4), ("M", 9)], 0, b"TTAGGGGGCATCGATT")]), {}))
    edge = [h([("M", 30, 3, 4, 20, 21)], 2)]  # events at 105, 106, 122, 123
    out.append(("window_edges", region(REF40, edge, window=(106, 122)), {}))
    out.append(("window_empty", region(REF40, edge, window=(107, 121)), {}))
    out.append(("widening_clipped_at_0", region(REF40, [h([("M", 30, 0, 1, 2)], 0)], ref_start=0, window=(0, 39), contig_length=40), dict(margin=2)))
    out.append(("widening_clipped_at_contig_end", region(REF40, [h([("M", 30, 27, 28, 29), ("D", 3), ("M", 4)], 3)], ref_start=60, contig_length=97),
                dict(margin=5)))
    out.append(("margin_0", region(REF40, span), dict(margin=0)))
    out.append(("no_haplotypes", region(REF40, []), {}))
    out.append(("one_failing_haplotype", region(REF40, [h([("M", 30, 5)], 2), h([("M", 6), ("N", 2), ("M", 6)], 2), h([("M", 6), ("I", b"T"), ("I", b"G"), ("M", 6)], 2)]), {}))
    return out


def random_region(rng, ref_len, n_haps, rate=0.08, ref_start=1000):
    """Haplotypes made from the reference by random edits, so CIGAR and bases agree."""
    ref = bytes(rng.choice(list(b"ACGT"), ref_len).astype(np.uint8))
    pool = []  # a few edit scripts shared between the haplotypes, so events repeat across them
    haps = []
    for _ in range(n_haps):
        if pool and rng.random() < 0.3:
            haps.append(pool[int(rng.integers(len(pool)))])
            continue
        start = int(rng.integers(0, 4))
        pos, script = start, []
        while pos < ref_len - 4:
            n = int(min(ref_len - 2 - pos, rng.integers(1, 40)))
            script.append(("M", n) + tuple(o for o in range(n) if rng.random() < rate))
            pos += n
            k = rng.random()
            if k < 0.35:
                script.append(("I", bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 5))).astype(np.uint8))))
            if 0.25 < k < 0.6 and pos + 8 < ref_len:
                d = int(rng.integers(1, 7))
                script.append(("D", d))
                pos += d
            if 0.55 < k < 0.62:
                script.append(("I", b"AT"))
        script.append(("M", 1))
        pool.append(build(ref, script, start))
        haps.append(pool[-1])
    lo, hi = ref_start + int(rng.integers(0, 10)), ref_start + ref_len - 1 - int(rng.integers(0, 10))
    return region(ref, haps, ref_start=ref_start, window=(lo, hi), contig_length=ref_start + ref_len + int(rng.integers(0, 4)))


def random_batches():
    """(name, regions, distance): batches of 1, 2 and 65 regions with 0 ... 65 haplotypes, references of 40 ... 300 bases."""
    rng = np.random.default_rng(20240607)
    counts = (0, 1, 2, 8, 63, 64, 65)
    out = [("one_region", [random_region(rng, 120, 8)], 0), ("two_regions", [random_region(rng, 40, 2), random_region(rng, 300, 65, 0.05)], 1)]
    out.append(("many_loci", [random_region(rng, 300, 8, 0.3)], 0))  # more than 64 loci, more than 64 events on a haplotype
    out.append(("65_regions", [random_region(rng, int(rng.integers(40, 301)), counts[i % 7], 0.04 + 0.02 * (i % 5)) for i in range(65)], 3))
    return out


def golden():
    return json.load(open(GOLDEN))


def census(regions, dist=0, include_spanning=True, margin=2):
    """What a set of regions exercises: counts by event kind, blocks, '*' alleles, flagged events, statuses."""
    c = dict(snp=0, mnp=0, insertion=0, deletion=0, block=0, star=0, flagged=0, events=0, loci_max=0, hap_events_max=0, multi_allelic=0, unmapped=0)
    status = {}
    for rg in regions:
        r = R.discover_region(rg["ref"], rg["ref_start"], rg["haps"], rg["window"], rg["contig_length"], dist, include_spanning, margin)
        status[r["status"]] = status.get(r["status"], 0) + 1
        c["events"] += len(r["events"])
        c["loci_max"] = max(c["loci_max"], len(r["events"]))
        for ev in r["events"]:
            c["star"] += R.SPAN_DEL in ev["kinds"]
            c["flagged"] += ev["flags"] != 0
            c["multi_allelic"] += len(ev["alleles"]) > 2
            c["unmapped"] += -1 in ev["hap_allele"]
        for m in r["maps"] or ():
            c["hap_events_max"] = max(c["hap_events_max"], len(m))
            for vc in m.values():
                simple = vc.vtype == R.INDEL and (len(vc.ref) == 1 or len(vc.alt) == 1) and vc.ref[0] == vc.alt[0]
                kind = "snp" if len(vc.ref) == 1 == len(vc.alt) else "mnp" if len(vc.ref) == len(vc.alt) and vc.vtype == R.MNP else \
                    "insertion" if simple and len(vc.ref) == 1 else "deletion" if simple else "block"
                c[kind] += 1
    c["status"] = status
    return c
