"""phmm_annotate_events beside phmm_genotype_likelihoods on genotype_bench's workloads A (1 024 regions x 128 reads x 8
haplotypes, 4 events each, 1 sample) and B (10 samples); prints one JSON line: per workload the time of both calls (host
clock around the synchronous call, after warm-up; median and min).  Every allele of an event is in its call; BQ reads the
batch's base qualities through one M element per read.  Both calls run in turn in every step, so a run under
`rocprofv3 --kernel-trace --stats` gives phmm_annotate_kernel and phmm_genotype_kernel on the same data and build.
usage: python tools/annotate_bench.py [--steps K] [--warmup W] [--workloads AB]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genotype_bench import workload  # noqa: E402
from lorikeet_amd import HipPairHMMEngine, genotype  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workloads", default="AB")
    a = ap.parse_args()
    eng = HipPairHMMEngine(0)
    out = {"tool": "annotate_bench", "steps": a.steps, "warmup": a.warmup}
    for name in a.workloads:
        b, lk, keep, start, end, sample, ev, ploidy, n_samples = workload(name)
        rng = np.random.default_rng(7)
        mapq = rng.integers(0, 61, size=b.n_reads).astype(np.uint8)
        calls = [list(range(ev.n_alleles(e))) for e in range(ev.n_events)]
        cigars = [np.array([int(n) << 4], np.uint32) for n in np.diff(b.read_off.astype(np.int64))]
        al = genotype.AlignedReads(b.read_off, b.base_q, cigars, start, ev.start + 2)
        err = np.full(ev.n_events, -10.0)
        gt = lambda: genotype.genotype_likelihoods(eng, b, lk, keep, start, end, sample, ev, ploidy=ploidy, n_samples=n_samples)  # noqa: E731
        an = lambda: genotype.annotate_events(eng, b, lk, keep, start, end, sample, mapq, ev, calls, err, n_samples=n_samples, aligned=al)  # noqa: E731
        for _ in range(a.warmup):
            gt()
            an()
        t_gt, t_an = [], []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            gt()
            t1 = time.perf_counter()
            res = an()
            t_gt.append(t1 - t0)
            t_an.append(time.perf_counter() - t1)
        out[name] = {"regions": int(b.n_regions), "events": int(ev.n_events), "samples": n_samples,
                     "call_alleles": int(sum(len(c) for c in calls)), "informative_reads": int(res.info_dp.sum()),
                     "annotate_call_ms_median": round(float(np.median(t_an)) * 1e3, 3), "annotate_call_ms_min": round(min(t_an) * 1e3, 3),
                     "genotype_call_ms_median": round(float(np.median(t_gt)) * 1e3, 3), "genotype_call_ms_min": round(min(t_gt) * 1e3, 3)}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
