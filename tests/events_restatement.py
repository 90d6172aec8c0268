"""Test infrastructure, not product code: a statement-by-statement restatement of the head of the reference's
assign_genotype_likelihoods, what tests/test_events_hip.py holds phmm_discover_events to.

  process_cigar_for_initial_events   EventMap::process_cigar_for_initial_events (src/haplotype/event_map.rs:86-246)
  add_vc, make_block                 :253-262, :274-344
  build_event_maps                   EventMap::build_event_maps_for_haplotypes (:361-408)
  get_overlapping_events             :429-464
  events_from_haplotypes             AssemblyBasedCallerUtils::get_variant_contexts_from_active_haplotypes
                                     (src/assembly/assembly_based_caller_utils.rs:633-658)
  replace_span_dels                  src/haplotype/haplotype_caller_genotyping_engine.rs:726-751
  make_merged                        make_merged_variant_context (assembly_based_caller_utils.rs:559-578) ->
                                     VariantContextUtils::simple_merge (src/model/variant_context_utils.rs:379-553) with
                                     determine_reference_allele (:872-916), resolve_incompatible_alleles and
                                     create_allele_mapping (:792-859), VariantContext::build / make_alleles
                                     (src/model/variant_context.rs:124-199)
  create_allele_mapper               assembly_based_caller_utils.rs:720-840
  expand_within_contig               src/utils/simple_interval.rs:137-147, IntervalUtils::trim_interval_to_contig
                                     (src/utils/interval_utils.rs:21-40)
  discover_region                    the loop of assign_genotype_likelihoods up to the allele map
                                     (haplotype_caller_genotyping_engine.rs:125-229)

Things restated as written, not as intended:
  * make_block calls get_type() on a build_from_vc copy of vc1 BEFORE it replaces the alleles: the block's cached type is the
    type of vc1's alleles (a SNP + insertion block stays a SNP; joined with a deletion it becomes an INDEL, computed from
    the alleles the first block had).  is_snp / is_simple_* of vc1 read vc1's cached type; get_overlapping_events too.
  * BaseUtils::is_regular_base is rust-bio's dna::alphabet(), "ACGTacgt": lower-case acgt IS regular, N and n are not.  The
    mismatch test compares raw bytes, ByteArrayAllele::new upper-cases them (src/model/byte_array_allele.rs:38-82): 'a'
    against 'A' proposes an event whose two alleles are equal, VariantContext::build's LinkedHashSet keeps one, and
    build_event_maps_for_haplotypes returns Err (:387-399) -- or make_block asserts is_biallelic first.
  * ByteArrayAllele equality is the bases alone: the merged allele set drops an alt that equals an earlier allele whatever
    its reference flag; when that leaves no reference allele make_alleles panics.
  * create_allele_mapper meets a haplotype's overlapping events in start order and stops at the first one that starts before
    the locus, so as written no haplotype is pushed into two lists (get_overlapping_events returns at most one event per
    start).  The restatement still counts the pushes and reports a second one as a flag.
  * sort_variant_contexts_by_priority sorts by the position of the source name, and the events arrive in haplotype order: the
    order stays.  Its sort is unstable; equal keys (two events of one haplotype) are kept in arrival order here.
"""
REGULAR = frozenset(b"ACGTacgt")
ACCEPTED = frozenset(b"ACGTNacgtnRYKMSWBDHVU")  # acceptable_allele_bases (byte_array_allele.rs:182-207)
NO_VARIATION, SNP, MNP, INDEL = 0, 1, 2, 3
OP_M, OP_I, OP_D, OP_N, OP_S, OP_H, OP_P, OP_EQ, OP_X = range(9)
OPS = "MIDNSHP=X"
OK, BAD_OPERATOR, BLOCK, MERGE, CIGAR_OVERRUN, ALLELES = 0, -1, -2, -3, -4, -5
PLAIN, SPAN_DEL = 0, 1
HAP_IN_TWO_ALLELES = 1
STAR = b"*"


class Panic(Exception):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


class VC:
    """loc.start / loc.end (closed), the alleles as VariantContext::build leaves them (reference first), the cached type."""

    def __init__(self, start, end, alleles, source=None):
        self.start, self.end, self.source = start, end, source
        self.alleles = []  # make_alleles behind a LinkedHashSet: equal bases once
        for a in alleles:
            if a.upper() not in self.alleles:
                self.alleles.append(a.upper())
        self.vtype = type_of(self.alleles)

    ref = property(lambda s: s.alleles[0])
    alt = property(lambda s: s.alleles[1])
    key = property(lambda s: (s.start, tuple(s.alleles)))

    def copy(self):
        c = VC(self.start, self.end, self.alleles, self.source)
        c.vtype = self.vtype
        return c


def type_of(alleles):
    """determine_type / type_of_biallelic_variant (variant_context.rs:1022-1086) for one or two alleles."""
    if len(alleles) == 1:
        return NO_VARIATION
    r, a = alleles
    return (SNP if len(a) == 1 else MNP) if len(r) == len(a) else INDEL


def is_simple_indel(vc):  # variant_context.rs:1135-1142, on the cached type
    return vc.vtype == INDEL and len(vc.alleles) == 2 and vc.ref[0] == vc.alt[0] and (len(vc.ref) == 1 or len(vc.alt) == 1)


def parse_cigar(text):
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append((OPS.index(ch), int(n)))
            n = ""
    return out


def process_cigar_for_initial_events(ref, ref_start, hap, cigar, hap_start, dist, source=None):
    ref_pos, ap, proposed = hap_start, 0, []
    for ci, (op, ln) in enumerate(cigar):
        if op == OP_I:
            if ref_pos > 0:
                if ref_pos - 1 >= len(ref):
                    raise Panic(CIGAR_OVERRUN)
                alleles, start, ref_byte = [], ref_start + ref_pos - 1, ref[ref_pos - 1:ref_pos]
                if ref_byte[0] in REGULAR:
                    alleles.append(ref_byte)
                if not (ci == 0 or ci == len(cigar) - 1):
                    if ap + ln > len(hap):
                        raise Panic(CIGAR_OVERRUN)
                    bases = ref_byte + hap[ap:ap + ln]
                    if all(b in REGULAR for b in bases):
                        alleles.append(bases)
                if len(alleles) == 2:
                    proposed.append(VC(start, start, alleles, source))
            ap += ln
        elif op == OP_S:
            ap += ln
        elif op == OP_D:
            if ref_pos > 0:
                if ref_pos + ln > len(ref):
                    raise Panic(CIGAR_OVERRUN)
                bases, start = ref[ref_pos - 1:ref_pos + ln], ref_start + ref_pos - 1
                if all(b in REGULAR for b in bases):
                    proposed.append(VC(start, start + ln, [bases, bases[:1]], source))
            ref_pos += ln
        elif op in (OP_M, OP_EQ, OP_X):
            if ref_pos + ln > len(ref) or ap + ln > len(hap):
                raise Panic(CIGAR_OVERRUN)
            mism = [o for o in range(ln) if ref[ref_pos + o] != hap[ap + o] and ref[ref_pos + o] in REGULAR and hap[ap + o] in REGULAR]
            while mism:
                start = end = mism.pop(0)
                while mism and mism[0] - end <= dist:
                    end = mism.pop(0)
                proposed.append(VC(ref_start + ref_pos + start, ref_start + ref_pos + end,
                                   [ref[ref_pos + start:ref_pos + end + 1], hap[ap + start:ap + end + 1]], source))
            ref_pos += ln
            ap += ln
        else:
            raise Panic(BAD_OPERATOR)
    return proposed


def make_block(vc1, vc2):
    if not (vc1.start == vc2.start and len(vc1.alleles) == 2):
        raise Panic(BLOCK)
    if vc1.vtype != SNP:
        if not ((is_simple_indel(vc1) and len(vc1.alt) == 1 and is_simple_indel(vc2) and len(vc2.ref) == 1) or
                (is_simple_indel(vc1) and len(vc1.ref) == 1 and is_simple_indel(vc2) and len(vc2.alt) == 1)):
            raise Panic(BLOCK)
    elif vc2.vtype == SNP:
        raise Panic(BLOCK)
    b = vc1.copy()
    b.vtype = type_of(vc1.alleles)  # b.get_type() on the copy of vc1's alleles, before they are replaced
    if vc1.vtype == SNP:
        if vc1.ref == vc2.ref:
            if len(vc2.alleles) < 2:
                raise Panic(BLOCK)
            ref, alt = vc1.ref, vc1.alt + vc2.alt[1:]
        else:
            ref, alt = vc2.ref, vc1.alt
            b.end = vc2.end
    else:
        ins, dele = (vc1, vc2) if len(vc1.ref) == 1 else (vc2, vc1)
        ref, alt = dele.ref, ins.alt
        b.end = dele.end
    b.alleles = [ref, alt]
    return b


def add_vc(m, vc):
    m[vc.start] = make_block(m[vc.start], vc) if vc.start in m else vc


def event_map(ref, ref_start, hap, cigar, hap_start, dist, source=None):
    """EventMap::new: the haplotype's events by start (a dict in ascending key order)."""
    m = {}
    for vc in process_cigar_for_initial_events(ref, ref_start, hap, cigar, hap_start, dist, source):
        add_vc(m, vc)
    return dict(sorted(m.items()))


def state_for_testing(vcs):
    m = {}
    for vc in vcs:
        add_vc(m, vc)
    return dict(sorted(m.items()))


def build_event_maps(ref, ref_start, haps, dist):
    """haps: (bases, cigar, hap_start).  The maps and the sorted start positions; Err becomes Panic(ALLELES)."""
    maps, starts = [], set()
    for i, (bases, cigar, hs) in enumerate(haps):
        m = event_map(ref, ref_start, bases, cigar, hs, dist, i)
        maps.append(m)
        starts.update(m)
        if any(len(vc.alleles) != 2 for vc in m.values()):
            raise Panic(ALLELES)
    return maps, sorted(starts)


def get_overlapping_events(m, loc):
    over = [vc for s, vc in m.items() if s <= loc and vc.end >= loc]
    has_ins = any(vc.vtype == INDEL and len(vc.ref) == 1 for vc in over)
    dels = [vc for vc in over if vc.vtype == INDEL and len(vc.alt) == 1 and vc.end == loc]
    if dels and has_ins:
        return [vc for vc in over if vc.key != dels[0].key]  # `*v != &deletion_events_ending_at_loc[0]`: loc and alleles
    return over


def events_from_haplotypes(loc, maps, include_spanning):
    seen, out = set(), []
    for m in maps:
        for vc in get_overlapping_events(m, loc):
            if (include_spanning or vc.start == loc) and vc.key not in seen:
                seen.add(vc.key)
                out.append(vc)
    return out


def replace_span_dels(vcs, ref_base, loc):
    out = []
    for vc in vcs:
        if vc.start != loc:
            vc = vc.copy()
            vc.start = vc.end = loc
            vc.alleles = [ref_base.upper(), STAR]
        out.append(vc)
    return out


def make_merged(vcs):
    """simple_merge: (start, end, alleles) or None."""
    if not vcs:
        return None
    vcs = sorted(vcs, key=lambda vc: vc.source if vc.source is not None else 0)  # stable; the sources are in order already
    ref = None
    for vc in vcs:  # determine_reference_allele
        if ref is None or len(ref) < len(vc.ref):
            ref = vc.ref
        elif len(ref) == len(vc.ref) and ref != vc.ref:
            raise Panic(MERGE)
    alleles, longest = [], vcs[0]  # (bases, is_ref)
    for vc in vcs:
        assert vc.start == longest.start
        if vc.end - vc.start > longest.end - longest.start:
            longest = vc
        if ref == vc.ref:
            values = [(vc.ref, True), (vc.alt, False)]
        else:  # create_allele_mapping, then the reference
            extra = ref[len(vc.ref):]
            values = [(vc.alt if vc.alt == STAR else vc.alt + extra, False), (ref, True)]
        for a in values:
            if a[0] not in [b[0] for b in alleles]:
                alleles.append(a)
    if sum(r for _, r in alleles) != 1:
        raise Panic(MERGE)  # make_alleles: no reference allele left
    alleles.sort(key=lambda a: not a[1])  # make_alleles: the reference to the front
    return longest.start, longest.end, [a for a, _ in alleles]


def create_allele_mapper(merged_alleles, loc, maps, emit_spanning_dels):
    """{allele index: [haplotype indices]} in the reference's insertion order."""
    result = {0: []}
    ref = merged_alleles[0]
    for i, a in enumerate(merged_alleles[1:], 1):
        result[i] = []
    position = lambda a: merged_alleles.index(a) if a in merged_alleles else None
    for h, m in enumerate(maps):
        spanning = get_overlapping_events(m, loc)
        if not spanning:
            result[0].append(h)
            continue
        for ev in spanning:
            if ev.start == loc:
                if len(ev.ref) == len(ref):
                    i = position(ev.alt)
                elif len(ev.ref) < len(ref):
                    i = position(ev.alt + ref[len(ev.ref):])
                else:
                    continue
                if i is not None:
                    result[i].append(h)
            else:
                i = position(STAR) if emit_spanning_dels else None
                result[0 if i is None else i].append(h)
                break
    return result


def expand_within_contig(start, end, padding, contig_length):
    assert contig_length >= 1
    return (0 if start < padding else start - padding), min(contig_length, end + padding)


def discover_region(ref, ref_start, haps, window, contig_length, dist=0, include_spanning=True, margin=2):
    """One region: dict(status, events=[dict(loc, vc_start, vc_end, start, end, alleles, kinds, hap_allele, flags)], maps)."""
    try:
        maps, starts = build_event_maps(ref, ref_start, haps, dist)
        events = []
        for loc in starts:
            if loc < window[0] or loc > window[1]:
                continue
            at_loc = events_from_haplotypes(loc, maps, include_spanning)
            merged = make_merged(replace_span_dels(at_loc, ref[loc - ref_start:loc - ref_start + 1], loc))
            if merged is None:
                continue
            vs, ve, alleles = merged
            mapper = create_allele_mapper(alleles, loc, maps, include_spanning)
            hap_allele, flags = [-1] * len(haps), 0
            for a, hs in mapper.items():
                for h in hs:
                    if hap_allele[h] == -1:
                        hap_allele[h] = a
            pushes = [sum(h in hs for hs in mapper.values()) for h in range(len(haps))]
            if any(p > 1 for p in pushes):  # first list pushed to, in the order the reference pushes
                flags |= HAP_IN_TWO_ALLELES
                hap_allele = [-1] * len(haps)
                for h, m in enumerate(maps):
                    hap_allele[h] = first_push(alleles, loc, m, include_spanning)
            s, e = expand_within_contig(vs, ve, margin, contig_length)
            events.append(dict(loc=loc, vc_start=vs, vc_end=ve, start=s, end=e, alleles=alleles,
                               kinds=[SPAN_DEL if a == STAR else PLAIN for a in alleles], hap_allele=hap_allele, flags=flags))
        return dict(status=OK, events=events, maps=maps)
    except Panic as p:
        return dict(status=p.status, events=[], maps=None)


def first_push(alleles, loc, m, emit_spanning_dels):
    """The first list the reference pushes the haplotype to: it walks the overlapping events in order."""
    spanning = get_overlapping_events(m, loc)
    if not spanning:
        return 0
    for ev in spanning:
        for a, hs in create_allele_mapper(alleles, loc, [{ev.start: ev}], emit_spanning_dels).items():
            if hs:
                return a
    return -1


def discover(regions, dist=0, include_spanning=True, margin=2):
    """Many regions -> the dense arrays of phmm_discover_events as Python lists (dict), regions being dicts with ref,
    ref_start, haps [(bases, cigar [(op, len)], hap_start)], window (start, end), contig_length."""
    out = dict(region_event_off=[0], region_status=[], event_region=[], event_allele_off=[0], event_start=[], event_end=[],
               event_loc=[], vc_start=[], vc_end=[], event_flags=[], event_hap_allele=[], allele_length=[], allele_kind=[],
               allele_bases_off=[0], allele_bases=b"", hap_event_off=[0], hap_event_start=[], hap_event_end=[],
               hap_event_ref_length=[], hap_event_alt_off=[0], hap_event_alt=b"", hap_event_type=[])
    for g, rg in enumerate(regions):
        r = discover_region(rg["ref"], rg["ref_start"], rg["haps"], rg["window"], rg["contig_length"], dist, include_spanning, margin)
        out["region_status"].append(r["status"])
        for ev in r["events"]:
            out["event_region"].append(g)
            out["event_allele_off"].append(out["event_allele_off"][-1] + len(ev["alleles"]))
            for k, name in (("start", "event_start"), ("end", "event_end"), ("loc", "event_loc"), ("vc_start", "vc_start"),
                            ("vc_end", "vc_end"), ("flags", "event_flags")):
                out[name].append(ev[k])
            out["event_hap_allele"] += ev["hap_allele"]
            for a, k in zip(ev["alleles"], ev["kinds"]):
                out["allele_length"].append(len(a))
                out["allele_kind"].append(k)
                out["allele_bases"] += a
                out["allele_bases_off"].append(len(out["allele_bases"]))
        out["region_event_off"].append(len(out["event_region"]))
        for h in range(len(rg["haps"])):
            for vc in (r["maps"][h].values() if r["maps"] else ()):
                out["hap_event_start"].append(vc.start)
                out["hap_event_end"].append(vc.end)
                out["hap_event_ref_length"].append(len(vc.ref))
                out["hap_event_alt"] += vc.alt
                out["hap_event_alt_off"].append(len(out["hap_event_alt"]))
                out["hap_event_type"].append(vc.vtype)
            out["hap_event_off"].append(len(out["hap_event_start"]))
    return out
