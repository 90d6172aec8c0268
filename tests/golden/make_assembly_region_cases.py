"""Writes assembly_region_cases.json: the grids and the expected values of the reference's own tests of
pop_ready_assembly_regions (tests/activity_profile_unit_tests.rs: make_active_region_cut_tests :611-787, region_creation_tests
:406-443), transcribed as data.  Run from the repository root: python tests/golden/make_assembly_region_cases.py"""
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
ACTIVE_PROB_THRESHOLD = 0.002          # :18
MAX_PROB_PROPAGATION_DISTANCE = 50     # :17
CONTIG_LENGTH = 63025520               # contig 20 of the b37 fixture the tests read their contig length from


def normal_distribution(mean, sd, x):  # src/utils/math_utils.rs normal_distribution
    return math.exp(-(x - mean) * (x - mean) / (2.0 * sd * sd)) / (sd * math.sqrt(2.0 * math.pi))


def make_gaussian(mean, rng, sigma):   # :545-554
    return [normal_distribution(mean, sigma, float(i)) + float(F32(ACTIVE_PROB_THRESHOLD)) for i in range(rng)]


def find_cut_site_for_two_max_peaks(probs, min_region_size):   # :556-570
    for i in range(len(probs) - 2, min_region_size, -1):
        if probs[i] < probs[i + 1] and probs[i] < probs[i - 1]:
            return i + 1
    return None


def short(p):
    """the shortest decimal that reads back as the same f32"""
    return float(str(F32(p)))


def grids():
    """One entry per (active_region_size, min_region_size) of the reference's loops (:619-624)."""
    out = []
    for size in (10, 12, 20, 30, 40):                          # :619
        for mn in (1, 5, 10):                                  # :620
            mx = (size * 2) // 3
            if mn >= mx:
                continue
            g = dict(size=size, min_region_size=mn, max_region_size=mx)
            g["flat"] = mx                                     # :625-636 ones; the expected size
            g["point"] = [min(end, mx) for end in range(1, size)]   # :638-651 `end` ones, end = 1 ..; the expected sizes
            g["increasing"] = dict(expected=mx, probs=[short(F32(1.0) * (F32(i) + F32(1.0)) / F32(size)) for i in range(size)])             # :653-671
            g["decreasing"] = dict(expected=mx, probs=[short(F32(1.0) - F32(1.0) * (F32(i) + F32(1.0)) / F32(size)) for i in range(size)])  # :673-692
            g["two_peaks"] = []                                # a subset of :694-736: size 12, every other peak pair
            if size == 12:
                for root_sigma in (1.0, 2.0, 3.0):
                    for p1 in range(0, size // 2, 2):
                        for p2 in range(size // 2 + 1, size, 2):
                            g1, g2 = make_gaussian(float(p1), size, root_sigma), make_gaussian(float(p2), size, root_sigma + 1.0)
                            probs = [F32(g1[i]) + F32(g2[i]) for i in range(size)]
                            cut = find_cut_site_for_two_max_peaks(probs, mn)
                            if cut is not None and cut < mx:
                                g["two_peaks"].append(dict(expected=max(cut, mn), probs=[short(x) for x in probs]))
            # :738-784 ones, 0.5 at first_min, 0.75 at second_min: row first_min - 1 holds the expected sizes for second_min =
            # first_min + 1 ..; the reference computes expected_cut and prints it, the call that would assert it is commented
            # out (:775-781)
            g["two_minima"] = []
            for first in range(1, size):
                row = []
                for second in range(first + 1, size):
                    if first + 1 < mn:
                        if first == second - 1:
                            expected = mx
                        else:
                            expected = mx if second + 1 > mx else (mx if second + 1 < mn else second + 1)
                    elif first + 1 > mx:
                        expected = mx
                    else:
                        expected = first + 1
                    row.append(expected)
                g["two_minima"].append(row)
            out.append(g)
    return out


def main():
    head = dict(source="tests/activity_profile_unit_tests.rs", active_prob_threshold=ACTIVE_PROB_THRESHOLD,
                max_prob_propagation=MAX_PROB_PROPAGATION_DISTANCE, contig_length=CONTIG_LENGTH,
                region_creation=dict(starts=[1, 10, 100, CONTIG_LENGTH - 100, CONTIG_LENGTH - 10], sizes=[1, 10, 100, 1000, 10000],
                                     max_region_sizes=[10, 50, 200], parts=[1, 2, 3, 4, 5, 7, 10, 11, 13],
                                     start_with_active=[True, False], min_region_size=1, extension=0))
    dump = lambda x: json.dumps(x, separators=(",", ":"))  # noqa: E731
    lines = ['"%s":%s' % (k, dump(v)) for k, v in head.items()]   # one key a line, one grid a line
    lines.append('"cut_grids":[\n' + ",\n".join(dump(g) for g in grids()) + "\n]")
    with open(os.path.join(HERE, "assembly_region_cases.json"), "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")


if __name__ == "__main__":
    main()
