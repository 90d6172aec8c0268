"""Builds tests/golden/subset_alleles_cases.json from the reference's own test file tests/allele_subsetting_utils_unit_tests.rs
(run where the reference tree is at hand: pass its root as the argument): every case of make_update_pls_sacs_and_ad_data
(:65-295) that carries PLs -- the genotype's log10 likelihoods before `as_pls`, the alleles kept, and for the cases that
subset the expected genotype's log10 likelihoods and GQ.  Only the data is extracted: the number literals, in source order,
with the line each case's original likelihoods come from.  The one case left out (`empty_gt`, :138-144) has no PLs."""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "subset_alleles_cases.json")
ALLELES = {"AC": [0, 1], "AG": [0, 2], "ACG": [0, 1, 2]}
NUMS = r"vec!\[([-0-9.,\s]*)\]"


def numbers(text):
    return [float(x) for x in text.replace("\n", " ").split(",") if x.strip()]


def main():
    src = os.path.join(sys.argv[1], "tests", "allele_subsetting_utils_unit_tests.rs")
    text = open(src).read()
    body = text[text.index("fn make_update_pls_sacs_and_ad_data"):text.index("fn test_that_filtering_works_correctly")]
    base = text.index("fn make_update_pls_sacs_and_ad_data")
    named = {}
    for m in re.finditer(r"let (\w+) =\s*(MathUtils::normalize_sum_to_one\()?" + NUMS, body):
        v = numbers(m.group(3))
        if m.group(2):  # normalize_sum_to_one (math_utils.rs:402-415): each value over the sum
            s = 0.0
            for x in v:
                s += x
            v = [x / s for x in v]
        named[m.group(1)] = v
    uses = []  # every from_log10_likelihoods(..).as_pls(), in source order
    for m in re.finditer(r"from_log10_likelihoods\(\s*(\w+|" + NUMS + r")\s*\)\s*\.as_pls\(\)", body):
        arg = m.group(1)
        uses.append((text.count("\n", 0, base + m.start()) + 1, named[arg] if arg in named else numbers(m.group(2))))
    kept = re.findall(r"vc_a[cg]\.alleles = (AC|AG)\b", body)
    gqs = [int(x) for x in re.findall(r"_expected\.gq = (\d+);", body)]
    assert len(uses) == 4 + 2 * 6 and len(kept) == 6 and len(gqs) == 6, (len(uses), kept, gqs)
    cases = []
    for line, v in uses[:4]:  # no selection: the alleles stay A, C and the genotypes are expected back as they are
        cases.append({"line": line, "ploidy": 2, "n_alleles": 2, "keep": ALLELES["AC"], "log10_likelihoods": v, "expected_log10_likelihoods": v,
                      "expected_gq": None})
    for k in range(6):
        (line, orig), (_, want) = uses[4 + 2 * k], uses[5 + 2 * k]
        ploidy = {3: 1, 10: 3}[len(orig)]
        cases.append({"line": line, "ploidy": ploidy, "n_alleles": 3, "keep": ALLELES[kept[k]], "log10_likelihoods": orig,
                      "expected_log10_likelihoods": want, "expected_gq": gqs[k]})
    json.dump({"source": "tests/allele_subsetting_utils_unit_tests.rs:65-295", "cases": cases}, open(OUT, "w"), indent=0)
    print(len(cases), "cases ->", OUT)


if __name__ == "__main__":
    main()
