"""phmm_trim_regions on events_bench's workload -- 1 024 regions of 8 haplotypes over a 300-base reference (random edits:
tests/events_cases.py's generator, seeded) with the reference haplotype in front, the generator's window as active span and the
whole reference as padded span -- and on the rank kernel's worst case: ONE region of 512 haplotypes over 16 384 bases that
differ only in their last 64 bases, so nearly every pair is compared to the end.  Ten calls each after warm-up; prints one JSON
line: what came out (regions with variation, failed regions, output haplotypes, duplicates) and the whole call on the host
clock (median and min).  The kernels' own times come from ONE run under
`rocprofv3 --kernel-trace --stats -- python tools/region_trim_bench.py` (events_hap_kernel and the six trim_*_kernel).
usage: python tools/region_trim_bench.py [--steps K] [--warmup W] [--regions N] [--no-worst]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import events_cases as K  # noqa: E402
from lorikeet_amd import HipPairHMMEngine, trim  # noqa: E402


def as_trim_region(r):
    """the generator's haplotypes start at base 0 .. 3 and end a few bases short: each gets the location its CIGAR covers, the
    region's padded span is what they all cover, the active span the generator's window inside it"""
    ref, rs = r["ref"], r["ref_start"]
    haps = [(ref, [(0, len(ref))], 0, (rs, rs + len(ref) - 1), True)]
    for b, c, s in r["haps"]:
        on_ref = sum(n for op, n in c if op in (0, 2, 7, 8))
        haps.append((b, c, s, (rs + s, rs + s + on_ref - 1), False))
    padded = (max(h[3][0] for h in haps), min(h[3][1] for h in haps))
    active = (max(r["window"][0], padded[0]), min(r["window"][1], padded[1]))
    return trim.Region(ref, rs, active, padded, haps)


def worst_region(rng, n_haps=512, ref_len=16384):
    ref = rng.choice(list(b"ACGT"), ref_len).astype(np.uint8)
    haps = [(bytes(ref), [(0, ref_len)], 0, (0, ref_len - 1), True)]
    for i in range(1, n_haps):
        b = ref.copy()
        for at in (ref_len - 64 + i % 60, ref_len - 64 + (i // 60) * 6 % 60):
            b[at] = b"ACGT"[(b"ACGT".index(bytes([b[at]])) + 1 + i % 3) % 4]
        haps.append((bytes(b), [(0, ref_len)], 0, (0, ref_len - 1), False))
    return trim.Region(bytes(ref), 0, (100, ref_len - 1), (0, ref_len - 1), haps)


def timed(eng, packed, padding, warmup, steps):
    t = []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        res = trim.trim_regions(eng, packed, 0, padding)
        if i >= warmup:
            t.append(time.perf_counter() - t0)
    return res, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--regions", type=int, default=1024)
    ap.add_argument("--no-worst", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(2024)
    packed = trim.pack([as_trim_region(K.random_region(rng, 300, 8, 0.02)) for _ in range(a.regions)])
    eng = HipPairHMMEngine(0)
    res, t = timed(eng, packed, trim.DEFAULT_PADDING, a.warmup, a.steps)
    out = {"tool": "region_trim_bench", "regions": a.regions, "haplotypes": 9, "reference_bases": 300, "steps": a.steps,
           "regions_with_variation": int((res["variation_present"] != 0).sum()), "failed_regions": int((res["region_status"] < 0).sum()),
           "output_haplotypes": res["n_out"], "duplicates": int((res["hap_fate"] == trim.FATE_DUPLICATE).sum()),
           "cut_in_deletion": int((res["hap_fate"] == trim.FATE_CUT_IN_DELETION).sum()), "output_bases": int(len(res["out_hap_bases"])),
           "call_ms_median": round(float(np.median(t)) * 1e3, 3), "call_ms_min": round(min(t) * 1e3, 3),
           "staged_in_bytes": int(sum(np.asarray(packed[k]).nbytes for k, _ in trim.INPUTS))}
    if not a.no_worst:
        wres, wt = timed(eng, trim.pack([worst_region(rng)]), (20000, 20000, 75, 25), a.warmup, a.steps)   # the whole region stays
        out.update(worst_haplotypes=512, worst_reference_bases=16384, worst_output_haplotypes=wres["n_out"],
                   worst_output_bases=int(len(wres["out_hap_bases"])), worst_call_ms_median=round(float(np.median(wt)) * 1e3, 3),
                   worst_call_ms_min=round(min(wt) * 1e3, 3))
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
