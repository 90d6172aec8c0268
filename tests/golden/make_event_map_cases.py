"""Builds tests/golden/event_map_cases.json from the reference's own test files (run where the reference tree is at hand: pass
its root as the argument).  Only inputs and expected results are recorded, the literals in source order:
  tests/event_map_unit_tests.rs
    test_mnps                      every row: reference, haplotype, CIGAR, the distances, the expected [ref, alt] pairs
    test_get_overlapping_events    every row: haplotype, CIGAR, locus, the expected alleles (null: no event); the reference
                                   bases and hap_start_wrt_ref the helper shares (:67-68), max_mnp_distance 1
    test_make_blocks               every row: first, second and expected [ref, alt]
  tests/assembly_based_caller_utils_unit_tests.rs
    get_event_mapper_data, get_variant_contexts_from_active_haplotypes_data
                                   the haplotypes of each call as the events of their event maps (start, end, ref, alt, type),
                                   the locus, the expected events in order; event_mapper_expected: the haplotypes
                                   get_event_mapper_data expects per allele index (:287-294) and the order it passes them in"""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "event_map_cases.json")
STR = r'"(\w+)"'


def strings(text):
    return re.findall(STR, text)


def main():
    root = sys.argv[1]
    text = open(os.path.join(root, "tests", "event_map_unit_tests.rs")).read()
    out = {}
    body = text[text.index("fn run_mnp_tests"):text.index("fn run_overlapping_events_tests")]
    out["test_mnps"] = []
    for m in re.finditer(r'test_mnps\(\s*"(\w+)",\s*"(\w+)",\s*"(\w+)",\s*vec!\[([\d,\s]+)\],\s*vec!\[(.*?)\],\s*\);', body, re.S):
        pairs = strings(m.group(5))
        out["test_mnps"].append(dict(ref=m.group(1), hap=m.group(2), cigar=m.group(3), distances=[int(x) for x in m.group(4).split(",") if x.strip()],
                                     expected=[pairs[i:i + 2] for i in range(0, len(pairs), 2)]))
    helper = text[text.index("fn test_get_overlapping_events"):text.index("fn test_make_blocks")]
    out["overlapping_ref"] = re.search(r'let ref_bases = "(\w+)"', helper).group(1)
    out["overlapping_hap_start"] = int(re.search(r"let hap_start_wrt_ref = (\d+)", helper).group(1))
    body = text[text.index("fn run_overlapping_events_tests"):text.index("fn run_test_blocks")]
    alleles = dict(re.findall(r'let (\w+) = ByteArrayAllele::new\("(\w+)"', body))
    out["test_get_overlapping_events"] = []
    for m in re.finditer(r'test_get_overlapping_events\(\s*"(\w+)",\s*"(\w+)",\s*(\d+),\s*(None|Some\(&(\w+)\)),\s*(None|Some\(&(\w+)\)),?\s*\);', body):
        out["test_get_overlapping_events"].append(dict(hap=m.group(1), cigar=m.group(2), loc=int(m.group(3)),
                                                       ref=alleles.get(m.group(5)), alt=alleles.get(m.group(7))))
    body = text[text.index("fn run_test_blocks"):]
    out["test_make_blocks"] = [[strings(a), strings(b), strings(c)] for a, b, c in
                               re.findall(r"test_make_blocks\(vec!\[(.*?)\], vec!\[(.*?)\], vec!\[(.*?)\]\);", body)]

    text = open(os.path.join(root, "tests", "assembly_based_caller_utils_unit_tests.rs")).read()
    out["active_haplotypes"] = []
    for fn, call in (("fn get_event_mapper_data", "test_get_event_mapper"),
                     ("fn get_variant_contexts_from_active_haplotypes_data", "test_get_variants_contexts_from_active_haplotypes")):
        body = text[text.index(fn):]
        body = body[:body.index("\n}\n") + 3]
        events = [(m.start(), m.group(1), m) for m in re.finditer(
            r'let (?:mut )?(\w+) = vec!\[\s*ByteArrayAllele::new\(b"(\w+)", true\),\s*ByteArrayAllele::new\(b"(\w+)", false\),?\s*\];', body)]
        events += [(m.start(), "snp_alleles", m) for m in re.finditer(r'let (ref_allele) = ByteArrayAllele::new\(b"(\w+)", true\);\s*let snp_allele = ByteArrayAllele::new\(b"(\w+)", false\);', body)]
        vcs = {}
        for m in re.finditer(r"let mut (\w+) = VariantContext::build\(20, (\d+), (\d+), (\w+)(?:\.clone\(\))?\);", body):
            al = max((e for e in events if e[0] < m.start() and e[1] == m.group(4)), key=lambda e: e[0])[2]
            t = re.search(re.escape(m.group(1)) + r"\.(?:variant_type = Some|set_type)\(VariantType::(\w+)\)", body[m.end():]).group(1)
            vcs[m.group(1)] = dict(start=int(m.group(2)), end=int(m.group(3)), ref=al.group(2), alt=al.group(3), type=t)
        maps = {"dummy": []}
        for m in re.finditer(r"(\w+)\s*\.set_event_map\(EventMap::state_for_testing\((?:Vec::new\(\)|vec!\[(.*?)\])\)\)", body, re.S):
            maps[m.group(1)] = [vcs[n] for n in re.findall(r"(\w+?)(?:\.clone\(\))?(?:,|$|\s)", m.group(2) or "") if n in vcs]
        for i, m in enumerate(re.finditer(call + r"\(\s*(.*?)\s*\);?\n", body, re.S)):
            args = m.group(1)
            if call == "test_get_event_mapper":
                loc = vcs["snp_vc"]["start"]
                haps = re.findall(r"(\w+)\.clone\(\)", args[args.index("vec!["):])
                expected = [vcs["snp_vc"]]
            else:
                loc = int(re.search(r",\s*(\d+),", args).group(1))
                first, second = args[:args.index(str(loc))], args[args.index(str(loc)):]
                haps = re.findall(r"(\w+)(?:\.clone\(\))?", first.replace("vec!", ""))
                haps = [h for h in haps if h in maps and h != "dummy"]  # `dummy` is an empty list of haplotypes
                expected = [vcs[n] for n in re.findall(r"&(\w+)", second)]
            out["active_haplotypes"].append(dict(name="%s_%d" % (call, i), loc=loc, haplotypes=[maps[h] for h in haps], expected=expected))
    # get_event_mapper_data builds its expectation in a loop over the two alleles of snp_alleles (:287-294): the allele equal
    # to snp_alleles[k] maps to one haplotype, the other allele to the other; the haplotypes go in in the order of the call
    body = text[text.index("fn get_event_mapper_data"):]
    m = re.search(r"if &snp_alleles\[(\d)\] == a \{\s*test1_expected_map\.insert\(i, vec!\[&(\w+)\]\);\s*\} else \{\s*"
                  r"test1_expected_map\.insert\(i, vec!\[&(\w+)\]\);", body)
    k = int(m.group(1))
    order = re.findall(r"(\w+)\.clone\(\)", re.search(r"test_get_event_mapper\(.*?vec!\[(.*?)\]", body, re.S).group(1))
    out["event_mapper_expected"] = {str(1 - k): [m.group(3)], str(k): [m.group(2)], "order": order}
    assert len(out["test_mnps"]) == 10 and len(out["test_get_overlapping_events"]) == 16 and len(out["test_make_blocks"]) == 7, out
    assert len(out["active_haplotypes"]) == 1 + 9, [c["name"] for c in out["active_haplotypes"]]
    json.dump(out, open(OUT, "w"), indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
