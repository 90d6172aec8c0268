"""The tail of the reference's assign_genotype_likelihoods restated statement by statement, in its own form: Python sets and
dicts of haplotype indices, lists of alleles, ranges for normalize_alleles.  No bitsets, no dense arrays: what
phmm_phase_calls computes on the device is compared with this (tests/test_phase_hip.py), and a shared mistake is unlikely.
  make_annotated_call's trim      src/haplotype/haplotype_caller_genotyping_engine.rs:451-489
  trim_alleles, do_trim_alleles   src/model/variant_context_utils.rs:956-1108
  normalize_alleles               src/reads/alignment_utils.rs:585-675
  the called haplotypes           src/haplotype/haplotype_caller_genotyping_engine.rs:394-405
  phase_calls and below           src/assembly/assembly_based_caller_utils.rs:975-1348
  determine_type                  src/genotype/genotype_builder.rs:399-441
The reference has no test of phase_calls, trim_alleles or normalize_alleles: the restatement is pinned by reading, and
tests/test_phase_oracle.py holds it to expectations derived by hand from the cited lines.
A haplotype is its index in the region: the reference's HashSet<Haplotype> compares bases, and a region's haplotypes differ.
CENSUS counts the branches a run takes (tests/test_phase_oracle.py asserts that the GPU case sets reach each of them)."""
from collections import Counter

CENSUS = Counter()
PHASE_01, PHASE_10 = ("0|1", 1), ("1|0", 0)   # PhaseGroup: (description, alt_allele_index)


class Allele:
    """ByteArrayAllele (src/model/byte_array_allele.rs:6-94): equality is by bases; a symbolic allele has length 0."""
    def __init__(self, bases, is_ref=False):
        self.bases = bytes(bases).upper()
        self.is_ref = is_ref
        self.is_symbolic = self.bases.startswith(b"<") and self.bases.endswith(b">")

    def __len__(self):
        return 0 if self.is_symbolic else len(self.bases)

    def __eq__(self, other):
        return other is not None and self.bases == other.bases

    def __hash__(self):
        return hash(self.bases)

    def __repr__(self):
        return self.bases.decode() + ("*ref" if self.is_ref else "")


class VariantContext:
    """what the functions below read of one: loc.start / loc.end, the alleles (the reference first), the genotypes as lists of
    alleles (None = a no-call allele)"""
    def __init__(self, start, end, alleles, genotypes=()):
        self.start, self.end, self.alleles = start, end, list(alleles)
        self.genotypes = [list(g) for g in genotypes]
        self.is_phased = [False] * len(self.genotypes)
        self.attributes = [dict() for _ in self.genotypes]

    def get_alternate_alleles(self):
        return self.alleles[1:]


# ---- alignment_utils.rs:585-675 -------------------------------------------------------------------------------------------------
def last_base_on_right_is_same(sequences, bounds):
    last_base_on_right = sequences[0][bounds[0][1] - 1]
    return all(sequences[n][bounds[n][1] - 1] == last_base_on_right for n in range(len(sequences)))


def first_base_on_left_is_same(sequences, bounds):
    first_base_on_left = sequences[0][bounds[0][0]]
    return all(sequences[n][bounds[n][0]] == first_base_on_left for n in range(len(sequences)))


def next_base_on_left_is_same(sequences, bounds):
    next_base_on_left = sequences[0][bounds[0][0] - 1]
    return all(sequences[n][bounds[n][0] - 1] == next_base_on_left for n in range(len(sequences)))


def index(seq, i):
    """a Rust slice index: a negative one is a panic, not Python's wrap-around"""
    assert 0 <= i < len(seq), "index out of bounds"
    return seq[i]


class Checked:
    """a sequence whose indexing panics where Rust's would"""
    def __init__(self, seq):
        self.seq = seq

    def __getitem__(self, i):
        return index(self.seq, i)


def normalize_alleles(sequences, bounds, max_shift, trim):
    """bounds: [start, end) pairs as two-element lists, changed in place.  Returns (start_shift, end_shift)."""
    assert sequences and len(sequences) == len(bounds)
    assert all(max_shift <= b[0] for b in bounds), "maxShift goes past the start of a sequence"
    sequences = [Checked(s) for s in sequences]
    start_shift = end_shift = 0
    min_size = min(b[1] - b[0] for b in bounds)
    while trim and min_size > 0 and last_base_on_right_is_same(sequences, bounds):
        for b in bounds:
            b[1] -= 1
        min_size -= 1
        end_shift += 1
    while trim and min_size > 0 and first_base_on_left_is_same(sequences, bounds):
        for b in bounds:
            b[0] += 1
        min_size -= 1
        start_shift -= 1
    while start_shift < max_shift and next_base_on_left_is_same(sequences, bounds) and last_base_on_right_is_same(sequences, bounds):
        CENSUS["normalize: the shift loop moved"] += 1
        for b in bounds:
            b[0] -= 1
            b[1] -= 1
        start_shift += 1
        end_shift += 1
    return start_shift, end_shift


# ---- variant_context_utils.rs:956-1108 ------------------------------------------------------------------------------------------
def trim_alleles(input_vc, trim_forward, trim_reverse):
    if len(input_vc.alleles) <= 1 or any(len(a) == 1 and not a.is_symbolic for a in input_vc.alleles):
        CENSUS["trim: one allele or an allele of length 1"] += 1
        return input_vc
    sequences = [a.bases for a in input_vc.alleles if not a.is_symbolic]
    ranges = [[0, len(a)] for a in input_vc.alleles if not a.is_symbolic]
    if len(sequences) < len(input_vc.alleles):
        CENSUS["trim: a symbolic allele kept"] += 1
    shifts = normalize_alleles(sequences, ranges, 0, True)
    end_trim = shifts[1]
    start_trim = -shifts[0]
    empty_allele = any(r[1] - r[0] == 0 for r in ranges)
    restore_one_base_at_end = empty_allele and start_trim == 0
    restore_one_base_at_start = empty_allele and start_trim > 0
    CENSUS["trim: restore_one_base_at_end"] += restore_one_base_at_end
    CENSUS["trim: restore_one_base_at_start"] += restore_one_base_at_start
    end_bases_to_clip = end_trim - 1 if restore_one_base_at_end else end_trim
    start_bases_to_clip = start_trim - 1 if restore_one_base_at_start else start_trim
    return do_trim_alleles(input_vc, (start_bases_to_clip if trim_forward else 0) - 1, end_bases_to_clip if trim_reverse else 0)


def do_trim_alleles(input_vc, fwd_trim_end, rev_trim):
    if fwd_trim_end == -1 and rev_trim == 0:
        return input_vc
    CENSUS["trim: bases left the end"] += 1
    alleles = []
    for a in input_vc.alleles:
        if a.is_symbolic:
            alleles.append(a)
        else:
            lo, hi = fwd_trim_end + 1, len(a) - rev_trim
            assert 0 <= lo <= hi <= len(a), "slice out of range"
            alleles.append(Allele(a.bases[lo:hi], a.is_ref))
    # update_genotypes_with_mapped_alleles: every allele of a genotype becomes its trimmed self
    trimmed = {a: t for a, t in zip(input_vc.alleles, alleles)}
    genotypes = [[None if a is None else trimmed.get(a, a) for a in g] for g in input_vc.genotypes]
    start = input_vc.start + fwd_trim_end + 1
    return VariantContext(start, start + len(alleles[0]) - 1, alleles, genotypes)


def reverse_trim_alleles(input_vc):
    return trim_alleles(input_vc, False, True)


def make_annotated_call(merged_alleles_list_size_before_possible_trimming, call, trim=True):
    """haplotype_caller_genotyping_engine.rs:482-488 (the annotation itself is phmm_annotate_events')"""
    if not trim or len(call.alleles) == merged_alleles_list_size_before_possible_trimming:
        return call
    return reverse_trim_alleles(call)


# ---- assembly_based_caller_utils.rs:975-1348 ------------------------------------------------------------------------------------
def is_site_specific_alt_allele(a):
    return not (a.is_ref or a.bases == b"<NON_REF>" or a.bases == b"<*>" or a.bases == b"*")


def is_biallelic_with_one_site_specific_alternate_allele(vc):
    return sum(1 for a in vc.get_alternate_alleles() if is_site_specific_alt_allele(a)) == 1


def get_site_specific_alt_allele(call):
    return next((a for a in call.get_alternate_alleles() if is_site_specific_alt_allele(a)), None)


def construct_haplotype_mapping(original_calls, called_haplotypes, event_maps):
    """event_maps[h]: the events of haplotype h as (start, [alternate alleles])"""
    haplotype_map = {}
    for idx, call in enumerate(original_calls):
        if not is_biallelic_with_one_site_specific_alternate_allele(call):
            n = sum(1 for a in call.get_alternate_alleles() if is_site_specific_alt_allele(a))
            CENSUS["mapping: no site-specific alt" if n == 0 else "mapping: several site-specific alts"] += 1
            for a in call.get_alternate_alleles():
                CENSUS["mapping: '*' in an unmapped call"] += a.bases == b"*"
                CENSUS["mapping: <NON_REF> in an unmapped call"] += a.bases == b"<NON_REF>"
            haplotype_map[idx] = set()
        else:
            alt = get_site_specific_alt_allele(call)
            if alt is None:
                haplotype_map[idx] = set()
            else:
                haplotype_map[idx] = {h for h in called_haplotypes
                                      if any(start == call.start and alt in alts for start, alts in event_maps[h])}
    return haplotype_map


def construct_phase_set_mapping(original_calls, haplotype_map):
    haplotypes_with_called_variants = set()
    for hs in haplotype_map.values():
        haplotypes_with_called_variants |= hs
    total_available_haplotypes = len(haplotypes_with_called_variants)
    phase_set_mapping = {}
    num_calls = len(original_calls)
    unique_counter = 0
    for i in range(max(num_calls - 1, 0)):
        haplotypes_with_call = haplotype_map.get(i)
        if haplotypes_with_call is None or not haplotypes_with_call:
            CENSUS["link: empty set"] += 1
            continue
        call_is_on_all_alt_haps = len(haplotypes_with_call) == total_available_haplotypes
        # created empty and only ever retain()ed below: it stays empty, so the middle clause is false for every non-empty comp
        call_haplotypes_available_for_phasing = set()
        for j in range(i + 1, num_calls):
            haplotypes_with_comp = haplotype_map.get(j)
            if haplotypes_with_comp is None or not haplotypes_with_comp:
                continue
            comp_is_on_all_alt_haps = len(haplotypes_with_comp) == total_available_haplotypes
            first = len(haplotypes_with_call) == len(haplotypes_with_comp) and all(h in haplotypes_with_call for h in haplotypes_with_comp)
            middle = call_is_on_all_alt_haps and all(h in call_haplotypes_available_for_phasing for h in haplotypes_with_comp)
            assert not middle
            if first or middle or comp_is_on_all_alt_haps:
                CENSUS["link: together"] += 1
                CENSUS["link: together by |Sj| == total alone"] += not first
                if i not in phase_set_mapping:
                    if j in phase_set_mapping:
                        CENSUS["link: abort"] += 1
                        phase_set_mapping.clear()
                        return phase_set_mapping
                    CENSUS["link: new group"] += 1
                    phase_set_mapping[i] = (unique_counter, PHASE_01)
                    phase_set_mapping[j] = (unique_counter, PHASE_01)
                    call_haplotypes_available_for_phasing = {h for h in call_haplotypes_available_for_phasing if h in haplotypes_with_comp}
                    unique_counter += 1
                elif j not in phase_set_mapping:
                    CENSUS["link: join with i's phase"] += 1
                    phase_set_mapping[j] = phase_set_mapping[i]
                else:
                    CENSUS["link: both mapped"] += 1
            elif len(haplotypes_with_call) + len(haplotypes_with_comp) == total_available_haplotypes:
                intersection = haplotypes_with_call & haplotypes_with_comp
                if not intersection:
                    CENSUS["link: apart"] += 1
                    if i not in phase_set_mapping:
                        if j in phase_set_mapping:
                            CENSUS["link: abort"] += 1
                            phase_set_mapping.clear()
                            return phase_set_mapping
                        CENSUS["link: new group"] += 1
                        phase_set_mapping[i] = (unique_counter, PHASE_01)
                        phase_set_mapping[j] = (unique_counter, PHASE_10)
                        unique_counter += 1
                    elif j not in phase_set_mapping:
                        call_phase = phase_set_mapping[i]
                        CENSUS["link: join with the flipped phase"] += 1
                        CENSUS["link: flip of 1|0"] += call_phase[1] == PHASE_10
                        phase_set_mapping[j] = (call_phase[0], PHASE_10 if call_phase[1] == PHASE_01 else PHASE_01)
                    else:
                        CENSUS["link: both mapped"] += 1
                else:
                    CENSUS["link: unrelated"] += 1
            else:
                CENSUS["link: unrelated"] += 1
    return phase_set_mapping


def is_het(alleles):
    """determine_type == Het (genotype_builder.rs:399-441)"""
    if not alleles:
        return False
    saw_no_call = saw_multiple_alleles = False
    first_call_allele = None
    for allele in alleles:
        if allele is None:
            saw_no_call = True
        elif first_call_allele is None:
            first_call_allele = allele
        elif allele != first_call_allele:
            saw_multiple_alleles = True
    if saw_no_call:
        CENSUS["gt: no-call"] += 1
        return False
    CENSUS["gt: hom"] += not saw_multiple_alleles
    return saw_multiple_alleles


def create_unique_id(vc):
    return "%d_%s_%s" % (vc.start, vc.alleles[0].bases.decode(), vc.get_alternate_alleles()[0].bases.decode())


def phase_vc(vc, id_, phase_gt, phase_set_id):
    for n, alleles in enumerate(vc.genotypes):
        phased_alt_allele_index = phase_gt[1]
        CENSUS["gt: ploidy %d" % len(alleles)] += 1
        if is_het(alleles) and not is_site_specific_alt_allele(alleles[phased_alt_allele_index]):
            CENSUS["gt: het reversed"] += 1
            alleles.reverse()
        elif len(alleles) > 1 and all(a is not None for a in alleles) and len(set(alleles)) > 1:
            CENSUS["gt: het kept"] += 1
        vc.is_phased[n] = True
        vc.attributes[n].update(PID=id_, PGT=phase_gt[0], PS=phase_set_id)


def construct_phase_groups(original_calls, phase_set_mapping, index_to):
    leaders = {}
    for count in range(index_to):
        indexes = [i for i in range(len(original_calls)) if i in phase_set_mapping and phase_set_mapping[i][0] == count]
        assert len(indexes) >= 2, "Somehow we have a group of phased variants that has fewer than 2 members"
        unique_id = create_unique_id(original_calls[indexes[0]])
        phase_set_id = original_calls[indexes[0]].start
        for i in indexes:
            leaders[i] = indexes[0]
            phase_vc(original_calls[i], unique_id, phase_set_mapping[i][1], phase_set_id)
    return leaders


def phase_calls(calls, called_haplotypes, event_maps):
    """Returns what the device reports beside the calls themselves: the sets, the mapping (empty after an abort), the leaders,
    total, and whether the mapping was cleared."""
    haplotype_map = construct_haplotype_mapping(calls, called_haplotypes, event_maps)
    total = len(set().union(*haplotype_map.values())) if haplotype_map else 0
    aborts = CENSUS["link: abort"]
    phase_set_mapping = construct_phase_set_mapping(calls, haplotype_map)
    aborted = CENSUS["link: abort"] != aborts
    unique_counter_end_value = len({p[0] for p in phase_set_mapping.values()})
    leaders = construct_phase_groups(calls, phase_set_mapping, unique_counter_end_value)
    return haplotype_map, phase_set_mapping, leaders, total, aborted


# ---- one region, in the form tests/phase_cases.py builds ------------------------------------------------------------------------
def region(reg, n_samples, ploidy, trim=True, with_gt=True):
    """reg: dict(haps=[[(start, alt bytes), ...] per haplotype], events=[dict(start, alleles=[bytes], hap_allele=[int per
    haplotype], call=[allele indices] (empty: not called), gt=[[index into call or -1] * ploidy] * n_samples)]).
    Returns one dict per event with the names of phmm_phase_calls' outputs, and (total, aborted)."""
    n_haps = len(reg["haps"])
    event_maps = [[(start, [Allele(alt)]) for start, alt in h] for h in reg["haps"]]
    return_calls, called_haplotypes, called_events = [], set(), []
    for e, ev in enumerate(reg["events"]):
        if not ev["call"]:
            continue
        merged = [Allele(b, k == 0) for k, b in enumerate(ev["alleles"])]
        # create_allele_mapper's result: merged allele index -> its haplotypes
        allele_mapper = {}
        for h, a in enumerate(ev["hap_allele"]):
            if a >= 0:
                allele_mapper.setdefault(a, []).append(h)
        by_merged_index = {h for a in ev["call"] for h in allele_mapper.get(a, [])}
        alleles = [merged[a] for a in ev["call"]]
        genotypes = [[None if x < 0 else alleles[x] for x in g] for g in ev["gt"]] if with_gt else []
        assert all(len(g) == ploidy for g in genotypes) and (not with_gt or len(genotypes) == n_samples)
        start = ev["start"]
        call = VariantContext(start, start + len(merged[0]) - 1, alleles, genotypes)
        annotated_call = make_annotated_call(len(merged), call, trim)
        return_calls.append(annotated_call)
        called_events.append(e)
        by_position = set()
        for idx in range(len(call.alleles)):          # :394-405: the POSITION in the call's list keys the merged map
            a = allele_mapper.pop(idx, None)
            if a is not None:
                by_position.update(a)
        CENSUS["called: position-as-key differs from the merged index"] += by_position != by_merged_index
        called_haplotypes |= by_position
    haplotype_map, mapping, leaders, total, aborted = phase_calls(return_calls, called_haplotypes, event_maps)
    out = []
    for e, ev in enumerate(reg["events"]):
        if not ev["call"]:
            out.append(dict(call_rev_trim=0, call_end=-1, phase_n_haps=0, hap_in_call=[0] * n_haps, phase_group=-1, phase_gt=0,
                            phase_leader=-1, phase_set=-1, is_phased=[0] * n_samples, gt_phased=[[-1] * ploidy for _ in range(n_samples)]))
            continue
        i = called_events.index(e)
        vc = return_calls[i]
        ref_len = len(Allele(ev["alleles"][0], True))
        rev_trim = ref_len - len(vc.alleles[0])
        assert vc.start == ev["start"] and all(len(Allele(ev["alleles"][a])) - len(t) == rev_trim
                                               for a, t in zip(ev["call"], vc.alleles) if not t.is_symbolic)
        CENSUS["mapping: a trimmed allele matched"] += bool(rev_trim and haplotype_map[i])
        d = dict(call_rev_trim=rev_trim, call_end=vc.end, phase_n_haps=len(haplotype_map[i]),
                 hap_in_call=[int(h in haplotype_map[i]) for h in range(n_haps)], phase_group=-1, phase_gt=0, phase_leader=-1, phase_set=-1)
        if i in mapping:
            d.update(phase_group=mapping[i][0], phase_gt=0 if mapping[i][1] == PHASE_01 else 1,
                     phase_leader=called_events[leaders[i]], phase_set=return_calls[leaders[i]].start)
        d["is_phased"] = [int(x) for x in vc.is_phased] if with_gt else [0] * n_samples
        # back to indices into the call's list: a context's alleles are distinct
        d["gt_phased"] = [[-1 if a is None else vc.alleles.index(a) for a in g] for g in vc.genotypes] if with_gt else []
        out.append(d)
    return out, (total, aborted)
