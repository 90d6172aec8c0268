"""The regions tests/test_phase_oracle.py (CPU) and tests/test_phase_hip.py (GPU) share: built in the form
phase_restatement.region reads, packed into the dense arrays phmm_phase_calls takes, and the restatement's answer in the
layout of the call's outputs.  A region is dict(haps=[[(start, alt bytes), ...] per haplotype, ascending by start],
events=[dict(start, alleles, hap_allele, call, gt)]) -- see phase_restatement.region."""
import copy
import random

import numpy as np

import phase_restatement as R

STAR, NON_REF = b"*", b"<NON_REF>"
KIND = {STAR: 1, NON_REF: 2}
PER_EVENT = ("call_rev_trim", "call_end", "phase_n_haps", "phase_group", "phase_gt", "phase_leader", "phase_set")
DTYPES = dict(call_rev_trim=np.uint32, call_end=np.int64, phase_n_haps=np.uint32, hap_in_call=np.uint8, phase_group=np.int32,
              phase_gt=np.uint8, phase_leader=np.int32, phase_set=np.int64, region_alt_haps=np.uint32, region_phase_flags=np.uint32,
              is_phased=np.uint8, gt_phased=np.int32)


def event(start, alleles, hap_allele, call=None, gt=None):
    """call: the indices of the alleles the call keeps (None: all of them, (): not called)"""
    return dict(start=start, alleles=[bytes(a) for a in alleles], hap_allele=list(hap_allele),
                call=list(range(len(alleles))) if call is None else list(call), gt=gt)


def by_sets(n_haps, calls, first=100, step=7):
    """A region of biallelic SNP calls, call k at first + k * step carried by the haplotypes of the set calls[k]: every
    haplotype is allele 0 or 1 of every event, so all are called, and S_k is calls[k]."""
    haps = [[] for _ in range(n_haps)]
    events = []
    for k, s in enumerate(calls):
        start = first + k * step
        for h in sorted(s):
            haps[h].append((start, b"T"))
        events.append(event(start, [b"A", b"T"], [1 if h in s else 0 for h in range(n_haps)]))
    return dict(haps=haps, events=events)


def draw_gt(regions, n_samples, ploidy, seed):
    """the regions with genotypes drawn for every called event: hom-ref, het, hom-var, no-call and mixed ones, non-decreasing as
    phmm_assign_genotypes writes them"""
    rng = random.Random(seed)
    out = copy.deepcopy(regions)
    for reg in out:
        for ev in reg["events"]:
            if ev["gt"] is not None or not ev["call"]:
                continue
            C = len(ev["call"])
            ev["gt"] = []
            for _ in range(n_samples):
                how = rng.randrange(6)
                if how == 0 or C == 1:
                    g = [0] * ploidy
                elif how == 1:
                    g = [-1] * ploidy
                elif how == 2:
                    g = [rng.randrange(1, C)] * ploidy
                elif how == 3:
                    g = sorted([-1] + [rng.randrange(C) for _ in range(ploidy - 1)])
                else:
                    g = sorted([0] + [rng.randrange(C) for _ in range(ploidy - 1)])
                ev["gt"].append(g)
    return out


def pack(regions, n_samples=0, ploidy=0, with_gt=False):
    """The input arrays of phmm_phase_calls (the names of lorikeet_amd.phase.INPUTS, region_hap_off, the call lists, gt)."""
    off = lambda lens: np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.uint32)  # noqa: E731
    events = [ev for reg in regions for ev in reg["events"]]
    haps = [h for reg in regions for h in reg["haps"]]
    hap_events = [x for h in haps for x in h]
    alleles = [a for ev in events for a in ev["alleles"]]
    # <NON_REF> is symbolic: it takes no bytes, and its length is the reference's 0
    bases = [b"" if a == NON_REF else a for a in alleles]
    gt = None
    if with_gt:
        gt = np.full((len(events), n_samples, ploidy), -7, np.int32)   # (an event that is not called: never read)
        for e, ev in enumerate(events):
            if ev["call"]:
                gt[e] = np.array(ev["gt"], np.int32).reshape(n_samples, ploidy)
    hm = [x for reg in regions for ev in reg["events"] for x in ev["hap_allele"]]
    assert all(len(ev["hap_allele"]) == len(reg["haps"]) for reg in regions for ev in reg["events"])
    return dict(
        region_event_off=off([len(reg["events"]) for reg in regions]), region_hap_off=off([len(reg["haps"]) for reg in regions]),
        event_allele_off=off([len(ev["alleles"]) for ev in events]), event_hap_allele=np.array(hm, np.int32),
        vc_start=np.array([ev["start"] for ev in events], np.int64), allele_length=np.array([len(b) for b in bases], np.uint32),
        allele_kind=np.array([KIND.get(a, 0) for a in alleles], np.uint8), allele_bases_off=off([len(b) for b in bases]),
        allele_bases=np.frombuffer(b"".join(bases), np.uint8).copy(), hap_event_off=off([len(h) for h in haps]),
        hap_event_start=np.array([x[0] for x in hap_events], np.int64), hap_event_alt_off=off([len(x[1]) for x in hap_events]),
        hap_event_alt=np.frombuffer(b"".join(x[1] for x in hap_events), np.uint8).copy(),
        call_allele_off=off([len(ev["call"]) for ev in events]),
        call_allele=np.array([c for ev in events for c in ev["call"]], np.uint32), gt=gt)


def unpack(a, call_allele_off, call_allele, gt=None):
    """pack's inverse for arrays that come from elsewhere (a discover_events result as a dict, with region_hap_off): the regions
    in the restatement's form"""
    regions = []
    n_regions = len(a["region_event_off"]) - 1
    m = 0
    for g in range(n_regions):
        haps = []
        for k in range(int(a["region_hap_off"][g]), int(a["region_hap_off"][g + 1])):
            haps.append([(int(a["hap_event_start"][i]), bytes(a["hap_event_alt"][int(a["hap_event_alt_off"][i]):int(a["hap_event_alt_off"][i + 1])]))
                         for i in range(int(a["hap_event_off"][k]), int(a["hap_event_off"][k + 1]))])
        events = []
        for e in range(int(a["region_event_off"][g]), int(a["region_event_off"][g + 1])):
            alleles = []
            for x in range(int(a["event_allele_off"][e]), int(a["event_allele_off"][e + 1])):
                b0 = int(a["allele_bases_off"][x])
                alleles.append(NON_REF if a["allele_kind"][x] == 2 else bytes(a["allele_bases"][b0:b0 + int(a["allele_length"][x])]))
            call = [int(c) for c in call_allele[int(call_allele_off[e]):int(call_allele_off[e + 1])]]
            events.append(event(int(a["vc_start"][e]), alleles, [int(x) for x in a["event_hap_allele"][m:m + len(haps)]], call,
                                None if gt is None else np.asarray(gt)[e].tolist()))
            m += len(haps)
        regions.append(dict(haps=haps, events=events))
    return regions


def expected(regions, n_samples=0, ploidy=0, trim=True, with_gt=False):
    """The restatement's answer as the call's output arrays (is_phased and gt_phased None without gt)."""
    o = {k: [] for k in DTYPES}
    e0 = 0
    for reg in regions:
        per_event, (total, aborted) = R.region(copy.deepcopy(reg), n_samples, ploidy, trim, with_gt)
        for d in per_event:
            for k in PER_EVENT:
                o[k].append(d[k] + e0 if k == "phase_leader" and d[k] >= 0 else d[k])
            o["hap_in_call"] += d["hap_in_call"]
            if with_gt:
                o["is_phased"].append(d["is_phased"])
                o["gt_phased"].append(d["gt_phased"])
        o["region_alt_haps"].append(total)
        o["region_phase_flags"].append(int(aborted))
        e0 += len(reg["events"])
    out = {k: np.array(v, DTYPES[k]) for k, v in o.items()}
    out["is_phased"] = out["is_phased"].reshape(e0, n_samples) if with_gt else None
    out["gt_phased"] = out["gt_phased"].reshape(e0, n_samples, ploidy) if with_gt else None
    return out


# ---- the hand cases of tests/test_phase_oracle.py, which derives the expectation of each from the cited lines ------------------
def two_snps_on_one_haplotype():
    return by_sets(2, [{1}, {1}])


def two_snps_on_the_two_alt_haplotypes():
    return by_sets(2, [{0}, {1}])


def joins_in_both_directions():
    return by_sets(2, [{0}, {1}, {1}, {0}])


def on_all_alt_haplotypes():
    return by_sets(3, [{0}, {0, 1}])


def abort():
    return by_sets(3, [{0}, {1}, {0, 1, 2}])


def unmapped_calls():
    """two phased SNPs around a multi-allelic call, a '*'-only call and a <NON_REF> call"""
    reg = by_sets(3, [{1}, {1}], first=100, step=40)
    multi = event(110, [b"A", b"C", b"G"], [0, 1, 2])
    star = event(120, [b"A", STAR], [0, 1, 1])
    non_ref = event(130, [b"A", NON_REF], [0, 0, 0])
    reg["haps"][1] += [(110, b"C")]
    reg["haps"][2] += [(110, b"G")]
    for h in reg["haps"]:
        h.sort()
    reg["events"] = [reg["events"][0], multi, star, non_ref, reg["events"][1]]
    return reg


def deletion_and_snp(drop_deletion=True):
    """At 200 haplotype 1 deletes CG (ACG -> A) and haplotype 2 has the SNP A -> T, merged as ACG / A / TCG; a SNP at 210 on
    haplotypes 1 and 2 calls all three haplotypes.  With the deletion dropped the call at 200 is ACG / TCG."""
    haps = [[], [(200, b"A"), (210, b"C")], [(200, b"T"), (210, b"C")]]
    locus = event(200, [b"ACG", b"A", b"TCG"], [0, 1, 2], call=[0, 2] if drop_deletion else None)
    snp = event(210, [b"G", b"C"], [0, 1, 1])
    return dict(haps=haps, events=[locus, snp])


def position_as_key():
    """deletion_and_snp's locus alone: its call keeps the alleles {0, 2} of three, the positions 0 and 1 key the merged map, and
    haplotype 2 -- the one that carries the SNP -- is not called"""
    reg = deletion_and_snp()
    return dict(haps=[[x for x in h if x[0] == 200] for h in reg["haps"]], events=reg["events"][:1])


def trims():
    """calls that lost an allele (the dropped one is last), so make_annotated_call trims: a length-1 allele, restore_one_base_at_end,
    restore_one_base_at_start, a symbolic allele kept, and a call that was not cut down and is therefore not trimmed"""
    haps = [[], [(300, b"A"), (310, b"CA"), (320, b"AC"), (330, b"T"), (340, b"TCG")]]
    return dict(haps=haps, events=[
        event(300, [b"ACG", b"A", b"TCG"], [0, 1], call=[0, 1]),               # A has length 1: unchanged, and A matches
        event(310, [b"AC", b"CAC", b"GGAC"], [0, 1], call=[0, 1]),             # AC / CAC: both bases of AC go, one comes back
        event(320, [b"AC", b"ACC", b"GGG"], [0, 1], call=[0, 1]),              # AC / ACC: C goes, then A in front: A / AC
        event(330, [b"ACG", b"TCG", NON_REF, b"GGG"], [0, 1], call=[0, 1, 2]),  # ACG / TCG / <NON_REF> -> A / T / <NON_REF>
        event(340, [b"ACG", b"TCG"], [0, 1]),                                  # all alleles kept: no trim, TCG matches TCG
    ])


HAND = dict(two_snps_on_one_haplotype=two_snps_on_one_haplotype, two_snps_on_the_two_alt_haplotypes=two_snps_on_the_two_alt_haplotypes,
            joins_in_both_directions=joins_in_both_directions, on_all_alt_haplotypes=on_all_alt_haplotypes, abort=abort,
            unmapped_calls=unmapped_calls, deletion_and_snp=deletion_and_snp, position_as_key=position_as_key, trims=trims)


# ---- shapes: the pass and word boundaries of the haplotypes, the chunks of the link kernel's j ---------------------------------
HAP_COUNTS = (1, 2, 63, 64, 65, 128, 512)
CALL_COUNTS = (0, 1, 2, 64, 65, 130)


def hap_boundaries(n_haps):
    """the matching haplotypes in the last and the first lane of a pass, and at both ends of the region"""
    want = [{n_haps - 1}, {n_haps - 1}, {0, 64, 448}, {63, 127, 511}, {0, 64, 448}, {63, 127, 511}, {0}, set(range(0, n_haps, 3))]
    return by_sets(n_haps, [s for s in ({h for h in w if h < n_haps} for w in want) if s])


def call_chunks(n_calls, with_abort=False):
    """n_calls calls of which most have the empty set; the related ones lie a chunk of 64 apart from their i"""
    sets = [set() for _ in range(n_calls)]
    if n_calls >= 2:
        sets[0], sets[-1] = {0}, {0}                     # together, in the last chunk of i = 0
    if n_calls >= 64:
        sets[1], sets[40] = {1, 2}, {3}                  # unrelated to {0} while total is 4 ...
        sets[n_calls - 2] = {0, 3}                       # ... apart from {1, 2}, in another chunk than i = 1
    if with_abort:
        assert n_calls >= 130
        sets[2], sets[100] = {2}, {0, 1, 2, 3}           # on all alt haplotypes: mapped by i = 0, met again by i = 1, 98 calls on
    return by_sets(4, sets)


def seeded(seed):
    """2-12 haplotypes, 1-40 calls; a call's set is empty, an earlier one again (together), what an earlier one leaves of the
    haplotypes so far (apart), or anything"""
    rng = random.Random(seed)
    n_haps, n_calls = rng.randint(2, 12), rng.randint(1, 40)
    universe = set(rng.sample(range(n_haps), rng.randint(1, n_haps)))
    sets = []
    for _ in range(n_calls):
        how = rng.randrange(8)
        earlier = [s for s in sets if s]
        if how == 0:
            s = set()
        elif how in (1, 2) and earlier:
            s = set(rng.choice(earlier))
        elif how in (3, 4) and earlier:
            s = universe - rng.choice(earlier)
        elif how == 5:
            s = set(universe)
        else:
            s = set(rng.sample(sorted(universe), rng.randint(1, len(universe))))
        sets.append(s)
    reg = by_sets(n_haps, sets)
    # some calls lose their shape: a '*' beside the alt, <NON_REF> beside it, a second alt, an event that is not called
    for ev in reg["events"]:
        how = rng.randrange(10)
        if how == 0:
            ev["alleles"].append(STAR)
            ev["call"] = [0, 1, 2]
        elif how == 1:
            ev["alleles"].append(NON_REF)
            ev["call"] = [0, 1, 2]
        elif how == 2:
            ev["alleles"].append(b"G")
            ev["call"] = [0, 1, 2]
        elif how == 3:
            ev["call"] = []
        elif how == 4:                                   # a call that lost an allele: trimmed, but T has length 1
            ev["alleles"].append(b"G")
        elif how == 5:                                   # ... and one that lost the allele the haplotypes carry
            ev["alleles"].append(b"G")
            ev["call"] = [0, 2]
    return reg


SEEDS = tuple(range(1, 25))


def sets():
    """(name, regions) of every set the GPU tests run"""
    out = [("hand " + k, [f()]) for k, f in HAND.items()]
    out.append(("hand untrimmed locus", [deletion_and_snp(drop_deletion=False)]))
    out += [("haplotypes %d" % n, [hap_boundaries(n)]) for n in HAP_COUNTS]
    out += [("calls %d" % n, [call_chunks(n)]) for n in CALL_COUNTS]
    out.append(("calls 130 abort", [call_chunks(130, with_abort=True)]))
    out.append(("no haplotypes", [dict(haps=[], events=[event(5, [b"A", b"T"], [])])]))
    out.append(("seeded", [seeded(s) for s in SEEDS]))
    return out


GT_SHAPES = ((1, 1), (1, 2), (3, 2), (1, 3), (3, 3), (3, 1))   # (n_samples, ploidy)
