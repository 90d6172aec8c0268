"""Test infrastructure, not product code: a statement-by-statement restatement of what the reference's call_region
(src/haplotype/haplotype_caller_engine.rs:1194-1243) does with the assembler's haplotypes before a likelihood is computed,
what tests/test_region_trim_hip.py holds phmm_trim_regions to.

  overlaps, coord_overlaps           SimpleInterval::overlaps (src/utils/simple_interval.rs:341-343 -> :201-205), the override that
                                     region.get_span().overlaps(..) reaches; CoordMath::overlaps (:245-249), the three clauses
  get_variation_events               AssemblyResultSet::get_variation_events (src/assembly/assembly_result_set.rs:283-366): the
                                     event maps (tests/events_restatement.py) into a BTreeSet by VariantContext's Ord
                                     (src/model/variant_context.rs:69-82)
  find_repeated_substring .. get_num_tandem_repeat_units
                                     src/model/variant_context_utils.rs:205-225, :240-335, :151-194, :32-79;
                                     TandemRepeat::get_num_tandem_repeat_units (src/annotator/tandem_repeat.rs:16-26)
  trimmer_trim                       AssemblyRegionTrimmer::trim (src/assembly/assembly_region_trimmer.rs:61-131)
  trim_with_padded_span              src/assembly/assembly_region.rs:323-339
  get_bases_covering_ref_interval    src/reads/alignment_utils.rs:759-843, base by base as written
  trim_cigar                         :334-386 with by_reference; CigarBuilder from tests/finalize_restatement.py
  haplotype_trim                     Haplotype::trim (src/haplotype/haplotype.rs:149-236)
  trim_down_haplotypes, trim_to      assembly_result_set.rs:465-499, :398-440 with a real ordered map (OrderedMap below)
  trim_region, trim_batch            the whole of it for one region / for a batch, as the arrays phmm_trim_regions returns

Things restated as written, not as intended:
  * get_num_tandem_repeat_units returns Some only when `lengths` is EMPTY (:74): with one alternate allele it is None whatever
    the alleles.  find_repeated_substring tests every start, not every rep_length-th, so only homopolymers decompose.
  * TandemRepeat slices the reference bases from start + 1 - padded_span.start although they begin at the padded reference
    location: the offset is wrong, and the slice panics when the subtraction underflows or the index lies behind the bases.
  * trim_cigar builds with CigarBuilder::new(true): deletions at the ends of the trimmed CIGAR go, whatever the comment in
    Haplotype::trim says about keeping them.
  * Haplotype::new upper-cases the bases: equality and order of trimmed haplotypes are of the upper-cased bytes.
"""
import bisect

import events_restatement as EV
from finalize_restatement import CigarBuilder

OP_M, OP_I, OP_D, OP_N, OP_S, OP_H, OP_P, OP_EQ, OP_X = range(9)
VARIATION_SPAN, VARIATION_SET = 1, 2
DUPLICATE, CUT_IN_DELETION, EMPTY, ALL_INSERTION, NOT_TRIMMED = -1, -2, -3, -4, -5
LOCATION, LENGTH, OPERATOR, NOT_FOUND, BUILDER, REF_ELIMINATED, REPEAT_SLICE = -16, -17, -18, -19, -20, -21, -22
STATUS_NAMES = {LOCATION: "LOCATION", LENGTH: "LENGTH", OPERATOR: "OPERATOR", NOT_FOUND: "NOT_FOUND", BUILDER: "BUILDER",
                REF_ELIMINATED: "REF_ELIMINATED", REPEAT_SLICE: "REPEAT_SLICE"}
NONE32 = 0xFFFFFFFF
REACHED = set()   # the branches a run went through (the census of tests/test_region_trim_oracle.py)


def reach(name):
    REACHED.add(name)


class Panic(Exception):
    def __init__(self, status):
        Exception.__init__(self, STATUS_NAMES.get(status, str(status)))
        self.status = status


def consumes_read(op):   # cigar_utils.rs:105-115
    return op in (OP_M, OP_EQ, OP_X, OP_I, OP_S)


def consumes_ref(op):    # :117-127
    return op in (OP_M, OP_D, OP_N, OP_EQ, OP_X)


# ---- intervals ------------------------------------------------------------------------------------------------------------------
def overlaps(a, b, margin=0):          # simple_interval.rs:201-205 (contigs match), reached through :341-343
    return a[0] <= b[1] + margin and max(b[0] - margin, 0) <= a[1]


def coord_overlaps(start, end, start2, end2):   # :245-249
    return (start2 >= start and start2 <= end) or (end2 >= start and end2 <= end) or (start >= start2 and end <= end2)


def intersect(a, b):                   # :152-165
    assert overlaps(a, b), "The two intervals need to overlap"
    return (max(a[0], b[0]), min(a[1], b[1]))


# ---- events ---------------------------------------------------------------------------------------------------------------------
def get_variation_events(ref, ref_start, haps, dist):
    """haps: (bases, cigar, hap_start).  The BTreeSet as a list in its order; equal keys keep the first inserted.
    Raises EV.Panic with the event map's status."""
    maps, _ = EV.build_event_maps(ref, ref_start, haps, dist)      # regenerate_variation_events :327-337
    out = {}
    for m in maps:                                                  # get_all_variant_contexts :360-363
        for vc in m.values():
            key = (vc.start, len(vc.ref), vc.alt)                   # variant_context.rs:69-82 (one contig)
            if key in out:
                reach("event:equal_key")
                assert (out[key].end, out[key].vtype) == (vc.end, vc.vtype)   # equal keys: equal span and cached type
            else:
                out[key] = vc
    return [out[k] for k in sorted(out)]


# ---- tandem repeats ---------------------------------------------------------------------------------------------------------------
def find_repeated_substring(bases):    # variant_context_utils.rs:205-225
    for rep_length in range(1, len(bases)):
        candidate = bases[0:rep_length]
        all_match = True
        for start in range(rep_length, len(bases)):
            piece = bases[start:min(start + len(candidate), len(bases))]
            if candidate != piece:
                all_match = False
                break
        if all_match:
            return rep_length
    return 0


def find_number_of_repetitions(unit, test, leading):   # :240-335
    if len(test) == 0:
        return 0
    diff = len(test) - len(unit)
    starts = range(0, diff + 1, len(unit)) if leading else range(diff, -1, -len(unit))
    n = 0
    for start in starts:
        if test[start:start + len(unit)] == unit:
            n += 1
        else:
            return n
    return n


def get_num_tandem_repeat_units_main(ref_bases, alt_bases, remain):   # :151-194
    long_b = alt_bases if len(alt_bases) > len(ref_bases) else ref_bases
    unit_len = find_repeated_substring(long_b)
    if unit_len > 0:
        unit = long_b[0:unit_len]
        in_ref = find_number_of_repetitions(unit, ref_bases, True)
        count = [max(find_number_of_repetitions(unit, ref_bases + remain, True) - in_ref, 0),   # checked_sub(..).unwrap_or(0)
                 max(find_number_of_repetitions(unit, alt_bases + remain, True) - in_ref, 0)]
        return count, unit
    return None


def get_num_tandem_repeat_units(is_indel, ref_allele, alts, ref_without_pad):   # :32-79
    if not is_indel:
        return None
    ref_allele_bases = ref_allele[1:len(ref_allele)]
    repeat_unit, lengths = b"", []
    for allele_bases in alts:
        if len(allele_bases) > 1:
            result = get_num_tandem_repeat_units_main(ref_allele_bases, allele_bases[1:len(allele_bases)], ref_without_pad)
            if result is None:
                return None
            if result[0][0] == 0 or result[0][1] == 0:
                return None
            if not lengths:
                lengths.append(result[0][0])
            lengths.append(result[0][1])
            repeat_unit = result[1]
        else:
            return None
    if not lengths:                    # :74 -- only without an alternate allele
        return lengths, repeat_unit
    return None


def tandem_repeat_units(padded_span, vc, reference):   # tandem_repeat.rs:16-26
    start_index = vc.start + 1 - padded_span[0]
    if start_index < 0 or start_index > len(reference):   # usize underflow; &reference[start_index..]
        raise Panic(REPEAT_SLICE)
    return get_num_tandem_repeat_units(vc.vtype == EV.INDEL, vc.ref, [vc.alt], reference[start_index:])


# ---- the trimmer ------------------------------------------------------------------------------------------------------------------
def trimmer_trim(active, padded, variants, reference, padding):
    """(variant_span, padded_span) or (None, None).  padding: (snp, indel, str, max extension)."""
    snp, indel, strp = padding[0], padding[1], padding[2]
    in_region = [vc for vc in variants if overlaps(active, (vc.start, vc.end))]   # :74-77
    if not in_region:
        reach("span:none")
        return None, None
    min_start = min(vc.start for vc in in_region)
    max_end = max(vc.end for vc in in_region)
    variant_span = intersect((min_start, max_end), active)        # :93-94
    for vc in in_region:
        pad = snp
        if vc.vtype == EV.INDEL:       # vc.is_indel(): the cached type
            pad = indel
            units = tandem_repeat_units(padded, vc, reference)
            if units is not None:      # :103-108
                reach("span:str")
                pad = strp + max(units[0], default=0) * len(units[1])
            reach("span:indel")
        else:
            reach("span:snp")
        if vc.start < pad:
            reach("span:saturated")
        min_start = min(min_start, max(vc.start - pad, 0))         # saturating_sub
        max_end = max(max_end, vc.end + pad)
    padded_variant_span = intersect((min_start, max_end), padded)  # :119-120
    assert padded_variant_span[0] <= variant_span[0] and padded_variant_span[1] >= variant_span[1]   # :227-235
    return variant_span, padded_variant_span


def trim_with_padded_span(active, padded, span, padded_span):      # assembly_region.rs:328-329
    return intersect(active, span), intersect(padded, padded_span)


# ---- Haplotype::trim --------------------------------------------------------------------------------------------------------------
def get_bases_covering_ref_interval(ref_start, ref_end, bases, bases_start_on_ref, cigar):   # alignment_utils.rs:759-843
    assert ref_end >= ref_start
    if len(bases) != sum(n for op, n in cigar if consumes_read(op)):   # :772-779
        raise Panic(LENGTH)
    ref_pos, bases_pos, bases_start, bases_stop, done = bases_start_on_ref, 0, None, None, False
    iii = 0
    while iii < len(cigar) and not done:
        op, ln = cigar[iii]
        if op == OP_I:
            bases_pos += ln
            if ref_pos in (ref_start, ref_end + 1):
                reach("bases:insertion_at_cut")
        elif op in (OP_M, OP_X, OP_EQ):
            for _ in range(ln):
                if ref_pos == ref_start:
                    bases_start = bases_pos
                if ref_pos == ref_end:
                    bases_stop = bases_pos
                    done = True
                    break
                ref_pos += 1
                bases_pos += 1
        elif op == OP_D:
            for _ in range(ln):
                if ref_pos == ref_end or ref_pos == ref_start:
                    reach("bases:deletion_at_start" if ref_pos == ref_start else "bases:deletion_at_end")
                    return None
                ref_pos += 1
        else:
            raise Panic(OPERATOR)      # :818-820
        iii += 1
    if ref_pos == ref_start:
        if not done:
            reach("bases:start_behind_loop")
        bases_start = bases_pos
    if ref_pos == ref_end:
        if not done:
            reach("bases:stop_behind_loop")
        bases_stop = bases_pos
    if bases_start is None or bases_stop is None:
        raise Panic(NOT_FOUND)         # :833-838
    if bases_stop + 1 > len(bases):
        reach("bases:min_len")
    return bases[bases_start:min(bases_stop + 1, len(bases))]


def trim_cigar(cigar, start, end, by_reference):   # :334-386; the elements, or Panic
    assert end >= start
    b = CigarBuilder(True)
    element_end = 0
    for op, ln in cigar:
        element_start = element_end
        element_end = element_start + (ln if (consumes_ref(op) if by_reference else consumes_read(op)) else 0)
        if element_end < start or (element_end == start and element_start < start):
            continue
        elif element_start > end and element_end > end + 1:
            break
        if element_end == element_start:
            reach("cigar:zero_length_kept")
            overlap = ln
        else:
            overlap = min(end + 1, element_end) - max(start, element_start)
        if not b.add(op, overlap):     # .expect("Failed to add Cigar element")
            raise Panic(BUILDER)
    if not element_end >= end:         # "Cigar elements don't reach end position (inclusive)"
        raise Panic(NOT_FOUND)
    out = b.make()                     # make_and_record_deletions_removed_result (cigar_builder.rs:321-325)
    if out is None:
        raise Panic(BUILDER)
    return out


def trim_cigar_by_reference(cigar, start, end):    # :853
    return trim_cigar(cigar, start, end, True)


def trim_cigar_by_bases(cigar, start, end):        # :321-323
    return trim_cigar(cigar, start, end, False)


def haplotype_trim(hap, loc):
    """hap: (bases, cigar, hap_start, (loc start, loc end), is_ref) with the CIGAR as (op, length) pairs.  Returns the fate
    (CUT_IN_DELETION, EMPTY, ALL_INSERTION) or (bases, cigar, hap_start); raises Panic."""
    bases, cigar, hap_start, gl, _ = hap
    if not (gl[0] <= loc[0] and gl[1] >= loc[1]):   # haplotype.rs:159-163
        raise Panic(LOCATION)
    new_start = loc[0] - gl[0]
    new_stop = new_start + loc[1] - loc[0]
    new_bases = get_bases_covering_ref_interval(new_start, new_stop, bases, 0, cigar)
    if new_bases is None:
        return CUT_IN_DELETION
    if len(new_bases) == 0:            # :180-182
        reach("trim:empty")
        return EMPTY
    new_cigar = trim_cigar_by_reference(cigar, new_start, new_stop)
    leading = not consumes_ref(new_cigar[0][0])
    trailing = not consumes_ref(new_cigar[-1][0])
    first, last = (1 if leading else 0), len(new_cigar) - (1 if trailing else 0)
    if last <= first:                  # :202-205
        reach("trim:all_insertion")
        return ALL_INSERTION
    if leading or trailing:            # :211-223
        reach("trim:leading" if leading else "trim:trailing")
        b = CigarBuilder(False)
        for op, ln in new_cigar[first:last]:
            if not b.add(op, ln):      # add_all(..).expect
                raise Panic(BUILDER)
        new_cigar = b.make()
        if new_cigar is None:          # Err -> trim_down_haplotypes' "Unhandled Trimming error"
            raise Panic(BUILDER)
    reach("trim:ok")
    return bytes(new_bases).upper(), new_cigar, new_start + hap_start   # Haplotype::new upper-cases (byte_array_allele.rs:76)


# ---- the ordered map ----------------------------------------------------------------------------------------------------------------
class OrderedMap:
    """A BTreeMap keyed by Haplotype's Ord (haplotype.rs:269-284): length, then bytes unsigned; equality by bases."""

    def __init__(self):
        self.keys, self.items = [], []   # sorted (len, bases); (key fields, value)

    @staticmethod
    def k(bases):
        return (len(bases), bytes(bases))

    def contains_key(self, bases):
        i = bisect.bisect_left(self.keys, self.k(bases))
        return i < len(self.keys) and self.keys[i] == self.k(bases)

    def remove(self, bases):
        i = bisect.bisect_left(self.keys, self.k(bases))
        del self.keys[i], self.items[i]

    def insert(self, bases, item):
        """BTreeMap::insert: an equal key keeps the OLD key and takes the new value."""
        i = bisect.bisect_left(self.keys, self.k(bases))
        if i < len(self.keys) and self.keys[i] == self.k(bases):
            self.items[i] = (self.items[i][0], item[1])
        else:
            self.keys.insert(i, self.k(bases))
            self.items.insert(i, item)


def trim_down_haplotypes(span, haps):   # assembly_result_set.rs:465-499
    """-> the map's items in order as (trimmed (bases, cigar, start, is_ref), original index), and the fates by input index."""
    m = OrderedMap()
    fates = [None] * len(haps)
    member_of = {}
    for i, h in enumerate(haps):
        trimmed = haplotype_trim(h, span)          # Err: panic!("Unhandled Trimming error")
        if isinstance(trimmed, int):
            fates[i] = trimmed
            if h[4]:
                raise Panic(REF_ELIMINATED)        # :487-490
            continue
        bases, cigar, start = trimmed
        item = ((bases, cigar, start, bool(h[4])), i)
        member_of[i] = OrderedMap.k(bases)
        if m.contains_key(bases):
            if h[4]:
                reach("order:reference_replaces")
                m.remove(bases)
                m.insert(bases, item)
            else:
                reach("order:duplicate_dropped")
        else:
            m.insert(bases, item)
    rep = {OrderedMap.k(t[0]): i for t, i in m.items}
    for rank, (t, i) in enumerate(m.items):
        fates[i] = rank
    dup_of = [NONE32] * len(haps)
    for i, key in member_of.items():
        if fates[i] is None:
            fates[i], dup_of[i] = DUPLICATE, rep[key]
    return m.items, fates, dup_of


def trim_region(region, dist=0, padding=(20, 75, 75, 25)):
    """region: (ref, ref_start, active, padded, haps) with haps as lorikeet_amd.trim.Region lists them (CIGARs as strings or
    pairs).  Returns a dict: status, variation, the four spans, fates, dup_of, out (the trimmed haplotypes in order as
    (bases, cigar, start, is_ref, source)), ref_hap."""
    ref, ref_start, active, padded, haps = region
    haps = [(bytes(h[0]), EV.parse_cigar(h[1]) if isinstance(h[1], str) else list(h[1]), h[2], h[3], h[4]) for h in haps]
    r = dict(status=0, variation=0, variant=(0, 0), padded=(0, 0), new_active=(0, 0), new_padded=(0, 0),
             fates=[NOT_TRIMMED] * len(haps), dup_of=[NONE32] * len(haps), out=[], ref_hap=-1)
    try:
        variants = get_variation_events(bytes(ref), ref_start, [(h[0], h[1], h[2]) for h in haps], dist)
    except EV.Panic as e:              # call_region :1197-1204: the empty model
        reach("region:event_map_failed")
        r["status"] = e.status
        return r
    try:
        span, padded_span = trimmer_trim(active, padded, variants, bytes(ref), padding)
    except Panic as e:
        reach("region:" + STATUS_NAMES[e.status])
        r["status"] = e.status
        return r
    if span is None:                   # :1227-1233
        return r
    r["variation"] = VARIATION_SPAN
    r["variant"], r["padded"] = span, padded_span
    r["new_active"], r["new_padded"] = trim_with_padded_span(active, padded, span, padded_span)
    try:
        items, fates, dup_of = trim_down_haplotypes(r["new_padded"], haps)
    except Panic as e:
        reach("region:" + STATUS_NAMES[e.status])
        r["status"] = e.status
        return r
    variation_present = any(not h[4] for h in haps)                # regenerate_variation_events :340
    for (bases, cigar, start, is_ref), i in items:                 # trim_to :409-429
        if is_ref:
            r["ref_hap"] = len(r["out"])
        else:
            variation_present = True
        r["out"].append((bases, cigar, start, is_ref, i))
    for f in fates:
        reach("fate:%s" % (f if f < 0 else "rank"))
    r["variation"] |= VARIATION_SET if variation_present else 0
    r["fates"], r["dup_of"] = fates, dup_of
    return r


def trim_batch(regions, dist=0, padding=(20, 75, 75, 25)):
    """The arrays phmm_trim_regions returns for a list of regions, as plain lists under the names of include/phmm.h."""
    o = {k: [] for k in ("region_status", "variation_present", "variant_start", "variant_end", "padded_start", "padded_end",
                         "new_active_start", "new_active_end", "new_padded_start", "new_padded_end", "hap_fate", "hap_dup_of",
                         "out_hap_bases", "out_hap_cigar", "out_hap_start_wrt_ref", "out_hap_source", "out_hap_is_ref",
                         "out_region_ref_hap")}
    o.update(out_region_hap_off=[0], out_hap_off=[0], out_hap_cigar_off=[0])
    for region in regions:
        r = trim_region(region, dist, padding)
        o["region_status"].append(r["status"])
        o["variation_present"].append(r["variation"])
        for name, key in (("variant", "variant"), ("padded", "padded"), ("new_active", "new_active"), ("new_padded", "new_padded")):
            o[name + "_start"].append(r[key][0])
            o[name + "_end"].append(r[key][1])
        o["hap_fate"] += r["fates"]
        o["hap_dup_of"] += r["dup_of"]
        o["out_region_ref_hap"].append(r["ref_hap"])
        for bases, cigar, start, is_ref, source in r["out"]:
            o["out_hap_bases"] += list(bases)
            o["out_hap_off"].append(len(o["out_hap_bases"]))
            o["out_hap_cigar"] += [(n << 4) | op for op, n in cigar]
            o["out_hap_cigar_off"].append(len(o["out_hap_cigar"]))
            o["out_hap_start_wrt_ref"].append(start)
            o["out_hap_source"].append(source)
            o["out_hap_is_ref"].append(1 if is_ref else 0)
        o["out_region_hap_off"].append(len(o["out_hap_start_wrt_ref"]))
    return o
